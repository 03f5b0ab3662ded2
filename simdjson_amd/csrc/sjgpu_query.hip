// simdjson_amd/csrc/sjgpu_query.hip -- queries over device tapes: a batched dom::element::at_pointer (sjgpu_at_pointers_device) and the
// string column as offsets + characters (sjgpu_gather_strings_device).  Contract: include/sjgpu_query.h.  The same walk rooted at the cells of a
// column (sjgpu_at_pointers_from_cells_device, include/sjgpu_rows.h) is at the end of the kernels, and behind it the paths rooted the same way
// (sjgpu_at_paths_from_cells_device, include/sjgpu_lists.h), and the fields and sizes of the cells' containers (sjgpu_object_fields_from_cells_device,
// sjgpu_cell_sizes_device, include/sjgpu_fields.h).
//
// The walk.  K pointers x docs documents = K * docs CELLS; one lane walks one cell, the lanes of a workgroup take consecutive documents of ONE
// pointer: the column stores are coalesced, the workgroup's pointer -- its tokens as sj_query_program.h compiled them and its
// unescaped key bytes, 2.3 KiB at most -- is copied to LDS once and read from there at every step, and the K lanes that walk one document
// (in K workgroups) find the lines its first visitor brought in.  NDJSON records are tens to hundreds of tape words: a cooperative walk
// per document would idle most of a wave.
// What the reference does per step (dom/object-inl.h:104-147 + :246-254, dom/array-inl.h:94-121 + array::at, dom/element-inl.h:427-446)
// is here a look at the tag of the word the walk stands on and one of three readings of the token, all prepared on the host:
//   {   the token as a key: its code if the escape is invalid, else the first field whose key record has the token's length and bytes
//   [   the token as an index: its code, else the element with that ordinal
//   else (a scalar) the verdict on the rest of the pointer
// Siblings are stepped over in O(1): a container word carries the index behind its partner in its low 32 bits, a number is two words, everything
// else one.  The walk only ever looks at the tag of a word it ARRIVED at by such steps, so a number's value word is never taken for a tag.
// Keys: the record is [u32 length][bytes][0] at any byte of the string buffer; the length is compared first and bytes are read only when it
// agrees, eight at a time while eight remain and one by one behind them -- never a byte behind the key's own.
// Nothing is trusted beyond the table check the host ran (the table ascends and ends inside the arrays): an index that leaves the document's
// slice, a step that does not advance, a record that leaves the document's string slice end the walk as "not found" (20 / 19).
//
// The gather.  Lengths from the column straight into the caller's offsets array, the context's exclusive scan over it (enqueue_scan), a total
// in 64 bits beside it (per-block sums, then one workgroup), and a copy that is parallel over the OUTPUT: a lane owns 16 bytes of it, finds the cell of its first byte by a search
// in the offsets and follows the cells from there -- a string of 100 KiB is 6 400 lanes' work, not one lane's.
#include "sjgpu_device.h"
#include "sj_path_program.h"

namespace sjgpu {
namespace {

constexpr u32 QUERY_THREADS = 256;
constexpr u64 LOW32 = 0xFFFFFFFFull, PAYLOAD = 0x00FFFFFFFFFFFFFFull;

typedef u32 __attribute__((aligned(1))) u32_unaligned;
typedef u64 __attribute__((aligned(1))) u64_unaligned;

__device__ __forceinline__ bool is_number_tag(u32 t) { return t == 'l' || t == 'u' || t == 'd'; }
__device__ __forceinline__ bool is_container_tag(u32 t) { return t == '{' || t == '['; }

// the index behind the element that begins at word i (whose word is w); base: the document's first word.  A step that would not advance
// (a tape that is not one) returns `end`: the level is over.
__device__ __forceinline__ u64 behind(u64 i, u64 w, u64 base, u64 end) {
  const u32 t = u32(w >> 56);
  const u64 next = is_container_tag(t) ? base + (w & LOW32) : i + (is_number_tag(t) ? 2u : 1u);
  return next > i ? next : end;
}

__device__ __forceinline__ bool key_equals(const u8 *__restrict__ rec, const u8 *key /* LDS, 8-byte aligned */, u32 len) {
  u32 j = 0;
  for (; j + 8 <= len; j += 8) {
    if (*reinterpret_cast<const u64_unaligned *>(rec + j) != *reinterpret_cast<const u64 *>(key + j)) { return false; }
  }
  for (; j < len; j++) {
    if (rec[j] != key[j]) { return false; }
  }
  return true;
}

// One at_pointer: the tokens tok[0 .. n) asked of the element that begins at word `cur` (its word: w) -> 0 with the element found in cur / w, or the
// reference's code.  limit: the end of what surrounds the element (the document, or the container whose child it is); no level is followed beyond it.
// The loop of k_at_pointers and of every PTR / TAIL level of k_at_paths.
__device__ __forceinline__ u32 walk_tokens(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, const query_token *tok /* LDS */, u32 n, const u8 *keys /* LDS, 8-byte aligned */,
                                           u64 base, u64 limit, u64 str_base, u64 str_end, u64 &cur, u64 &w) {
  for (u32 t = 0; t < n; t++) {
    const u32 kind = u32(w >> 56);
    if (kind == '{') {
      if (tok[t].key_code) { return tok[t].key_code; }
      const u32 klen = tok[t].key_len;
      const u8 *key = keys + tok[t].key_off;
      u64 end = base + (w & LOW32) - 1u; // the closing word
      end = end < limit ? end : limit;
      u64 i = cur + 1u;
      bool found = false;
      while (i + 1u < end) { // a key word and the first word of its value
        const u64 kw = tape[i], vw = tape[i + 1u];
        const u64 rec = str_base + (kw & PAYLOAD);
        if (rec + 4u <= str_end) {
          const u32 len = *reinterpret_cast<const u32_unaligned *>(sbuf + rec);
          if (len == klen && rec + 4u + u64(len) <= str_end && key_equals(sbuf + rec + 4u, key, klen)) {
            found = true;
            cur = i + 1u;
            w = vw;
            break;
          }
        }
        i = behind(i + 1u, vw, base, end);
      }
      if (!found) { return QUERY_NO_SUCH_FIELD; }
    } else if (kind == '[') {
      if (tok[t].arr_code) { return tok[t].arr_code; }
      const u64 want = tok[t].arr_index;
      u64 end = base + (w & LOW32) - 1u;
      end = end < limit ? end : limit;
      u64 i = cur + 1u, ordinal = 0;
      bool found = false;
      while (i < end) {
        const u64 ew = tape[i];
        if (ordinal == want) {
          found = true;
          cur = i;
          w = ew;
          break;
        }
        ordinal++;
        i = behind(i, ew, base, end);
      }
      if (!found) { return QUERY_INDEX_OUT_OF_BOUNDS; }
    } else {
      return tok[t].scalar_code;
    }
  }
  return 0;
}

// the value word of a string cell whose tape word is w -- a string element, or an object's key (k_object_fields): (length << 32) | the absolute offset of its first byte
__device__ __forceinline__ u64 string_cell_value(const u8 *__restrict__ sbuf, u64 w, u64 str_base, u64 str_end) {
  const u64 rec = str_base + (w & PAYLOAD);
  const u32 len = rec + 4u <= str_end ? *reinterpret_cast<const u32_unaligned *>(sbuf + rec) : 0u;
  return (u64(len) << 32) | ((rec + 4u) & LOW32);
}

// the value word of a cell that holds the element at word `cur` (include/sjgpu_query.h); its tag is w >> 56
__device__ __forceinline__ u64 cell_value(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 cur, u64 w, u64 base, u64 doc_end, u64 str_base, u64 str_end) {
  const u32 kind = u32(w >> 56);
  if (is_number_tag(kind)) { return cur + 1u < doc_end ? tape[cur + 1u] : 0; }
  if (kind == 't') { return 1; }
  if (kind == '"') { return string_cell_value(sbuf, w, str_base, str_end); }
  if (is_container_tag(kind)) { return ((base + (w & LOW32)) << 32) | cur; }
  return 0;
}

// pointer qp of the program into the workgroup's LDS, by all of its lanes: the pointer's tokens (4 words of 8 bytes each) and its key area -- what is behind
// the last key is never compared.  Ends behind the barrier.  The prologue of k_at_pointers and of k_at_pointers_rooted.
__device__ __forceinline__ void stage_pointer(const u8 *__restrict__ prog, u32 tokens_at, u32 keys_at, const query_pointer &qp, query_token *s_tok /* LDS */, u64 *s_key /* LDS */) {
  const u64 *src = reinterpret_cast<const u64 *>(prog + tokens_at) + u64(qp.first_token) * (sizeof(query_token) / 8);
  u64 *dst = reinterpret_cast<u64 *>(s_tok);
  for (u32 j = threadIdx.x; j < qp.tokens * u32(sizeof(query_token) / 8); j += QUERY_THREADS) { dst[j] = src[j]; }
  u32 key_words = 0;
  if (qp.tokens) {
    const query_token last = reinterpret_cast<const query_token *>(prog + tokens_at)[qp.first_token + qp.tokens - 1u];
    key_words = (last.key_off + last.key_len + 7u) / 8u;
  }
  key_words = key_words < QUERY_KEY_AREA / 8 ? key_words : QUERY_KEY_AREA / 8;
  const u64 *ksrc = reinterpret_cast<const u64 *>(prog + keys_at + qp.keys_at);
  for (u32 j = threadIdx.x; j < key_words; j += QUERY_THREADS) { s_key[j] = ksrc[j]; }
  lds_writes_done();
  __syncthreads();
}

// grid: K rows of row_blocks workgroups, row k = pointer k (one dimension: at most 64 * 2^24 workgroups)
__global__ __launch_bounds__(QUERY_THREADS) void k_at_pointers(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, const doc_span_dev *__restrict__ table, u32 docs,
                                                             const u8 *__restrict__ prog, u32 tokens_at, u32 keys_at, u32 row_blocks, u64 *__restrict__ value, u8 *__restrict__ tag) {
  __shared__ query_token s_tok[QUERY_MAX_TOKENS];
  __shared__ u64 s_key[QUERY_KEY_AREA / 8];
  const u32 k = blockIdx.x / row_blocks, row_block = blockIdx.x - k * row_blocks;
  const query_pointer qp = reinterpret_cast<const query_pointer *>(prog)[k];
  stage_pointer(prog, tokens_at, keys_at, qp, s_tok, s_key);
  const u64 d64 = u64(row_block) * QUERY_THREADS + threadIdx.x;
  if (d64 >= docs) { return; }
  const u32 d = u32(d64);
  const uint4 a = *reinterpret_cast<const uint4 *>(table + d), b = *reinterpret_cast<const uint4 *>(table + d + 1u);
  const u64 base = a.z, doc_end = b.z; // the document's words: [base, doc_end)
  const u64 str_base = a.w, str_end = b.w;
  u32 code = qp.code;
  u64 cur = base + 1u; // the root: behind the root word
  u64 w = 0;
  if (!code) {
    if (cur < doc_end) { w = tape[cur]; } else { code = QUERY_NO_SUCH_FIELD; }
  }
  if (!code) { code = walk_tokens(tape, sbuf, s_tok, qp.tokens, reinterpret_cast<const u8 *>(s_key), base, doc_end, str_base, str_end, cur, w); }
  const u32 out_tag = code ? code : u32(w >> 56);
  const u64 out_value = code ? 0 : cell_value(tape, sbuf, cur, w, base, doc_end, str_base, str_end);
  const u64 cell = u64(k) * docs + d;
  tag[cell] = u8(out_tag);
  value[cell] = out_value;
}

// one thread per entry: does the table ascend and end inside the arrays?  (A table of docs + 1 entries costs a fraction of the walk it guards.)
__global__ __launch_bounds__(QUERY_THREADS) void k_query_check_table(const doc_span_dev *__restrict__ table, u32 docs, u64 tape_words, u64 string_bytes, u32 *__restrict__ bad) {
  const u64 d64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (d64 > docs) { return; }
  const u32 d = u32(d64);
  const uint4 a = *reinterpret_cast<const uint4 *>(table + d);
  bool wrong;
  if (d == docs) {
    wrong = a.z > tape_words || a.w > string_bytes;
  } else {
    const uint4 b = *reinterpret_cast<const uint4 *>(table + d + 1u);
    wrong = a.z > b.z || a.w > b.w;
  }
  if (wrong) { atomicOr(bad, 1u); }
}

// ---- the gather -------------------------------------------------------------------------------------------------------------------------------
struct gather_ctrl {
  u64 total;     // the sum of the lengths in 64 bits (the scan's words wrap at 2^32)
  u32 n_plus_1;  // docs + 1: the length of the scan
  u32 pad;
};

constexpr u32 GATHER_PER_THREAD = 8, GATHER_BLOCK = QUERY_THREADS * GATHER_PER_THREAD;
// offsets[d] = the length of cell d (a string inside the buffer) or 0; offsets[docs] = 0: the exclusive scan in place makes them the offsets.
// block_sums[block]: the lengths of the block's 2 048 cells in 64 bits (one atomic per wave on ONE word was 165 us for 862 116 cells)
__global__ __launch_bounds__(QUERY_THREADS) void k_gather_lengths(const u64 *__restrict__ value, const u8 *__restrict__ tag, u32 docs, u64 string_bytes,
                                                                u32 *__restrict__ offsets, u64 *__restrict__ block_sums) {
  __shared__ u64 s_sum[QUERY_THREADS / 64];
  const u64 first = u64(blockIdx.x) * GATHER_BLOCK + threadIdx.x;
  u64 sum = 0;
#pragma unroll
  for (u32 j = 0; j < GATHER_PER_THREAD; j++) {
    const u64 d64 = first + u64(j) * QUERY_THREADS;
    u32 len = 0;
    if (d64 < docs && tag[d64] == '"') {
      const u64 v = value[d64];
      const u64 at = v & LOW32, l = v >> 32;
      len = at + l <= string_bytes ? u32(l) : 0u;
    }
    if (d64 <= docs) { offsets[d64] = len; }
    sum += len;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { sum += __shfl_xor(sum, m); }
  if (lane_id() == 0) { s_sum[threadIdx.x >> 6] = sum; }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) { block_sums[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]; }
}

// one workgroup: the total, and the length of the scan
__global__ __launch_bounds__(QUERY_THREADS) void k_gather_total(const u64 *__restrict__ block_sums, u32 blocks, u32 docs, gather_ctrl *__restrict__ ctrl) {
  __shared__ u64 s_sum[QUERY_THREADS / 64];
  u64 sum = 0;
  for (u32 j = threadIdx.x; j < blocks; j += QUERY_THREADS) { sum += block_sums[j]; }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { sum += __shfl_xor(sum, m); }
  if (lane_id() == 0) { s_sum[threadIdx.x >> 6] = sum; }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) {
    ctrl->total = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    ctrl->n_plus_1 = docs + 1u;
    ctrl->pad = 0;
  }
}

constexpr u32 GATHER_CHUNK = 16;
// a lane: 16 bytes of the output, [chunk * 16, ...) of `total`
__global__ __launch_bounds__(QUERY_THREADS) void k_gather_copy(const u8 *__restrict__ sbuf, const u64 *__restrict__ value, const u32 *__restrict__ offsets, u32 docs, u64 total,
                                                             u8 *__restrict__ chars) {
  const u64 first = (u64(blockIdx.x) * QUERY_THREADS + threadIdx.x) * GATHER_CHUNK;
  if (first >= total) { return; }
  const u32 count = total - first < GATHER_CHUNK ? u32(total - first) : GATHER_CHUNK;
  // the cell of byte `first`: the LAST d with offsets[d] <= first (cells of no bytes in front of it share its offset and are passed over)
  u32 lo = 0, hi = docs; // offsets[0] = 0 <= first < total = offsets[docs]
  while (hi - lo > 1u) {
    const u32 mid = lo + (hi - lo) / 2u;
    if (offsets[mid] <= first) { lo = mid; } else { hi = mid; }
  }
  u32 d = lo;
  u64 cell_begin = offsets[d], cell_end = offsets[d + 1u];
  const u8 *src = sbuf + (value[d] & LOW32);
  u32 bytes[GATHER_CHUNK / 4] = {0, 0, 0, 0};
#pragma unroll
  for (u32 j = 0; j < GATHER_CHUNK; j++) {
    if (j < count) {
      const u64 pos = first + j;
      while (pos >= cell_end && d + 1u < docs) { // (total = offsets[docs] > pos: a cell with bytes lies ahead)
        d++;
        cell_begin = cell_end;
        cell_end = offsets[d + 1u];
        src = sbuf + (value[d] & LOW32);
      }
      bytes[j / 4] |= u32(src[pos - cell_begin]) << (8u * (j & 3u));
    }
  }
  u8 *dst = chars + first;
  if (count == GATHER_CHUNK && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
    *reinterpret_cast<uint4 *>(dst) = make_uint4(bytes[0], bytes[1], bytes[2], bytes[3]);
  } else {
#pragma unroll
    for (u32 j = 0; j < GATHER_CHUNK; j++) {
      if (j < count) { dst[j] = u8(bytes[j / 4] >> (8u * (j & 3u))); }
    }
  }
}

// ---- the paths (include/sjgpu_paths.h) ---------------------------------------------------------------------------------------------------------
// One lane walks one cell (path k, document d) twice: once to count its matches (FILL = false), once -- behind the scan of the counts -- to write them
// (FILL = true).  The recursion of at_path_with_wildcard is an iterative depth-first walk over the path's LEVELS (sj_path_program.h): `have` says that
// the element at cur / w waits for level L; otherwise the topmost frame hands out its next child, or is popped.  A frame is pushed per WILD level that
// meets a container with children: (cursor of the next child's value, end of the level), document-relative, in LDS as [frame][lane] -- a per-lane array
// indexed by the stack pointer would live in scratch memory.  The frames' levels and kinds (object: a key word lies in front of every value) are eight
// bytes of one register.  A container's end is cut to the end of the frame it was reached from, so the children of two siblings never overlap and a
// cell's work stays linear in the words of its document whatever the tape says.
// path ph of the program into the workgroup's LDS, by all of its lanes: its levels, its tokens and its key area.  Ends behind the barrier.  The prologue of
// k_at_paths and of k_at_paths_rooted.
__device__ __forceinline__ void stage_path(const u8 *__restrict__ prog, u32 levels_at, u32 tokens_at, u32 keys_at, const path_header &ph, path_level *s_lev /* LDS */,
                                           query_token *s_tok /* LDS */, u64 *s_key /* LDS */) {
  const u32 tid = threadIdx.x;
  const u32 n_lev = ph.levels < PATH_MAX_LEVELS ? ph.levels : PATH_MAX_LEVELS, n_tok = ph.tokens < PATH_MAX_TOKENS ? ph.tokens : PATH_MAX_TOKENS;
  const u64 *lsrc = reinterpret_cast<const u64 *>(prog + levels_at) + u64(ph.first_level) * (sizeof(path_level) / 8);
  u64 *ldst = reinterpret_cast<u64 *>(s_lev);
  for (u32 j = tid; j < n_lev * u32(sizeof(path_level) / 8); j += QUERY_THREADS) { ldst[j] = lsrc[j]; }
  const u64 *src = reinterpret_cast<const u64 *>(prog + tokens_at) + u64(ph.first_token) * (sizeof(query_token) / 8);
  u64 *dst = reinterpret_cast<u64 *>(s_tok);
  for (u32 j = tid; j < n_tok * u32(sizeof(query_token) / 8); j += QUERY_THREADS) { dst[j] = src[j]; }
  u32 key_words = 0;
  if (n_tok) {
    const query_token last = reinterpret_cast<const query_token *>(prog + tokens_at)[ph.first_token + n_tok - 1u];
    key_words = (last.key_off + last.key_len + 7u) / 8u;
  }
  key_words = key_words < QUERY_KEY_AREA / 8 ? key_words : QUERY_KEY_AREA / 8;
  const u64 *ksrc = reinterpret_cast<const u64 *>(prog + keys_at + ph.keys_at);
  for (u32 j = tid; j < key_words; j += QUERY_THREADS) { s_key[j] = ksrc[j]; }
  lds_writes_done();
  __syncthreads();
}

// One at_path_with_wildcard: the levels s_lev[0 .. levels) asked of the element that begins at word `cur` (its word: w).  outer: the end of what surrounds the
// element (the document, or the root cell's own end); no level is followed beyond it.  base / doc_end / str_base / str_end: the four bounds of the element's
// document.  FILL: the matches go to value / tag[out .. out_end); else they are counted.  code: the status, set at level 0 only.  The walk of k_at_paths and of
// k_at_paths_rooted.
template <bool FILL>
__device__ __forceinline__ void walk_levels(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, const path_level *s_lev /* LDS */, u32 levels, const query_token *s_tok /* LDS */,
                                            const u8 *keys /* LDS, 8-byte aligned */, u32 (*s_cur)[QUERY_THREADS] /* LDS */, u32 (*s_end)[QUERY_THREADS] /* LDS */, u64 cur, u64 w,
                                            u64 outer, u64 base, u64 doc_end, u64 str_base, u64 str_end, u32 &count, u32 &code, u64 out, u64 out_end, u64 *__restrict__ value,
                                            u8 *__restrict__ tag) {
  const u32 tid = threadIdx.x;
  auto emit = [&](u64 at, u64 ew) {
    if (FILL) {
      if (out < out_end) { // never at or beyond the next cell's first match, whatever the tape says
        tag[out] = u8(ew >> 56);
        value[out] = cell_value(tape, sbuf, at, ew, base, doc_end, str_base, str_end);
        out++;
      }
    } else {
      count++;
    }
  };
  u32 L = 0, sp = 0;
  u64 frames = 0; // byte s: the level of frame s, bit 7: the frame walks an object
  bool have = true;
  for (;;) {
    if (have) {
      have = false;
      const u32 kind = u32(w >> 56);
      if (!is_container_tag(kind)) { continue; } // a scalar contributes nothing at any level, and is no error
      const u64 limit = sp ? base + s_end[sp - 1u][tid] : outer;
      const path_level lv = s_lev[L];
      if (lv.kind == PATH_PTR || lv.kind == PATH_TAIL) {
        const u32 c = walk_tokens(tape, sbuf, s_tok + lv.first_token, lv.tokens, keys, base, limit, str_base, str_end, cur, w);
        if (lv.kind == PATH_PTR) {
          if (!c && L + 1u < levels) { L++; have = true; }
        } else if (c) {
          if (L == 0) { code = c; }
        } else {
          emit(cur, w);
        }
      } else if (lv.kind == PATH_WILD || lv.kind == PATH_WILD_LAST) {
        const u32 obj = kind == '{' ? 1u : 0u;
        u64 end = base + (w & LOW32);
        end = end > cur ? end - 1u : cur; // the closing word
        end = end < limit ? end : limit;
        u64 i = cur + 1u + obj; // the first child's value
        if (lv.kind == PATH_WILD_LAST) {
          while (i < end) {
            const u64 ew = tape[i];
            emit(i, ew);
            i = behind(i, ew, base, end) + obj;
          }
        } else if (i < end && sp < PATH_MAX_WILDS && L + 1u < levels) {
          s_cur[sp][tid] = u32(i - base);
          s_end[sp][tid] = u32(end - base);
          frames = (frames & ~(0xFFull << (8u * sp))) | (u64(L | (obj << 7)) << (8u * sp));
          sp++;
        }
      } else if (L == 0) {
        code = QUERY_INVALID_JSON_POINTER; // ERR22
      }
    } else {
      if (sp == 0) { break; }
      const u32 f = u32(frames >> (8u * (sp - 1u))) & 0xFFu;
      const u64 end = base + s_end[sp - 1u][tid], i = base + s_cur[sp - 1u][tid];
      if (i < end) {
        cur = i;
        w = tape[i];
        const u64 next = behind(i, w, base, end) + (f >> 7);
        s_cur[sp - 1u][tid] = u32((next < end ? next : end) - base);
        L = (f & 31u) + 1u;
        have = true;
      } else {
        sp--;
      }
    }
  }
}

// what the count leaves: the cell's count and status, the scan's last entry, the workgroup's sum in 64 bits.  The epilogue of k_at_paths<false> and of
// k_at_paths_rooted<false>; lanes: the cells of one path (documents, or roots)
__device__ __forceinline__ void paths_count_done(bool active, u64 cell, u32 count, u32 code, u32 lanes, u32 row_blocks, u32 *__restrict__ offsets, u8 *__restrict__ status,
                                                 u64 *__restrict__ block_sums, u64 *s_sum /* LDS */) {
  const u32 tid = threadIdx.x;
  if (active) {
    offsets[cell] = code ? 0u : count;
    status[cell] = u8(code);
    if (cell == 0) { offsets[u64(gridDim.x / row_blocks) * lanes] = 0; } // the scan's last entry: the total lands there
  }
  u64 sum = code ? 0u : count;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { sum += __shfl_xor(sum, m); }
  if (lane_id() == 0) { s_sum[tid >> 6] = sum; }
  lds_writes_done();
  __syncthreads();
  if (tid == 0) { block_sums[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]; }
}

// grid: K rows of row_blocks workgroups, row k = path k
template <bool FILL>
__global__ __launch_bounds__(QUERY_THREADS) void k_at_paths(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, const doc_span_dev *__restrict__ table, u32 docs,
                                                          const u8 *__restrict__ prog, u32 levels_at, u32 tokens_at, u32 keys_at, u32 row_blocks, u32 *__restrict__ offsets,
                                                          u8 *__restrict__ status, u64 *__restrict__ block_sums, u64 *__restrict__ value, u8 *__restrict__ tag) {
  __shared__ query_token s_tok[PATH_MAX_TOKENS];
  __shared__ u64 s_key[QUERY_KEY_AREA / 8];
  __shared__ path_level s_lev[PATH_MAX_LEVELS];
  __shared__ u32 s_cur[PATH_MAX_WILDS][QUERY_THREADS], s_end[PATH_MAX_WILDS][QUERY_THREADS];
  __shared__ u64 s_sum[QUERY_THREADS / 64];
  const u32 k = blockIdx.x / row_blocks, row_block = blockIdx.x - k * row_blocks, tid = threadIdx.x;
  const path_header ph = reinterpret_cast<const path_header *>(prog)[k];
  stage_path(prog, levels_at, tokens_at, keys_at, ph, s_lev, s_tok, s_key);
  const u64 d64 = u64(row_block) * QUERY_THREADS + tid;
  const bool active = d64 < docs;
  const u64 cell = u64(k) * docs + d64;
  u32 count = 0, code = 0;
  u64 out = 0, out_end = 0; // FILL: the cell's matches are value / tag[out .. out_end)
  bool go = active;
  if (FILL && active) {
    out = offsets[cell];
    out_end = offsets[cell + 1u];
    go = out < out_end; // (a cell without matches, or with a status, has nothing to write)
  }
  if (go) {
    const u32 d = u32(d64);
    const uint4 a = *reinterpret_cast<const uint4 *>(table + d), b = *reinterpret_cast<const uint4 *>(table + d + 1u);
    const u64 base = a.z, doc_end = b.z; // the document's words: [base, doc_end)
    const u64 str_base = a.w, str_end = b.w;
    const u64 cur = base + 1u; // the root: behind the root word
    const u64 w = cur < doc_end ? tape[cur] : 0; // (no root: a tag that is no container's)
    walk_levels<FILL>(tape, sbuf, s_lev, ph.levels, s_tok, reinterpret_cast<const u8 *>(s_key), s_cur, s_end, cur, w, doc_end, base, doc_end, str_base, str_end, count, code, out,
                      out_end, value, tag);
  }
  if (FILL) { return; }
  paths_count_done(active, cell, count, code, docs, row_blocks, offsets, status, block_sums, s_sum);
}

// ---- the paths, wide (include/sjgpu_paths.h: sjgpu_at_paths_wide_device) --------------------------------------------------------------------------
// The same cells, breadth first: the elements that wait for level L of a path -- of ALL documents -- are one ascending list of tape indices (the FRONTIER),
// and a level turns one frontier into the next.  PTR / TAIL: one lane per element (walk_tokens), the survivors compacted in order.  WILD / WILD_LAST: the
// words between the frontier's containers and their closing words are laid end to end (the scanned extents: the RANGE SPACE), one lane per word of it; a
// word is a child of its container when it begins an element (its HEAD bit) one nesting level below the container.  Both come from the ANNOTATION, made
// once per call for the whole tape:
//   head   a word is a number's second word (raw bits, any byte on top) exactly when the word in front of it is a head tagged l, u or d.  Without a walk:
//          behind a word whose top byte is NOT one of the three comes a head, whatever that word was -- a payload is followed by a head, and a head that is
//          no number has one word --, and from there heads and payloads alternate while the top bytes keep looking like numbers.  So with mark(j) = j + 1
//          for a word whose top byte is none of l u d, else 0, and m = the largest mark in front of word i: i is a head iff i - m is even.  The running
//          maximum is carried across a lane's four words, the wave (shuffles), the workgroup (LDS) and the workgroups (k_wide_ann_summary, k_wide_ann_carry:
//          a two-level pass, nobody waits for anybody); every document begins with an `r`, so no run crosses into a document.
//   depth  the exclusive sum over the heads of +1 for { [ and -1 for } ] (enqueue_scan); only differences of two depths are ever looked at.
// Elements of one frontier lie side by side (every level descends the same number of steps), so a container's words end in front of the next element of
// the frontier: the extents are cut there, which changes nothing on a tape and keeps the range space within tape_words on anything else.
constexpr u32 WIDE_LANE_WORDS = 4, WIDE_SHARE = QUERY_THREADS * WIDE_LANE_WORDS; // a lane's and a workgroup's share of the annotation

__device__ __forceinline__ u32 umax32(u32 a, u32 b) { return a > b ? a : b; }
__device__ __forceinline__ u32 wide_mark(u64 w, u64 i) { return is_number_tag(u32(w >> 56)) ? 0u : u32(i) + 1u; }
// the document of tape word idx: the LAST d with tape_begin[d] <= idx (idx at or behind tape_begin[0], docs >= 1)
__device__ __forceinline__ u32 wide_doc_of(const doc_span_dev *__restrict__ table, u32 docs, u32 idx) {
  u32 lo = 0, hi = docs;
  while (hi - lo > 1u) {
    const u32 mid = lo + (hi - lo) / 2u;
    if (table[mid].tape_begin <= idx) { lo = mid; } else { hi = mid; }
  }
  return lo;
}
// the container of word r of the range space: the LAST e with start[e] <= r (start[0] = 0; containers without words share their successor's start)
__device__ __forceinline__ u32 wide_parent_of(const u32 *__restrict__ start, u32 F, u32 r) {
  u32 lo = 0, hi = F;
  while (hi - lo > 1u) {
    const u32 mid = lo + (hi - lo) / 2u;
    if (start[mid] <= r) { lo = mid; } else { hi = mid; }
  }
  return lo;
}

// share_last[b] = the largest mark of workgroup b's words
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_ann_summary(const u64 *__restrict__ tape, u32 n, u32 *__restrict__ share_last) {
  __shared__ u32 s_max[QUERY_THREADS / 64];
  const u64 i0 = u64(blockIdx.x) * WIDE_SHARE + u64(threadIdx.x) * WIDE_LANE_WORDS;
  u32 m = 0;
#pragma unroll
  for (u32 j = 0; j < WIDE_LANE_WORDS; j++) {
    if (i0 + j < n) { m = umax32(m, wide_mark(tape[i0 + j], i0 + j)); }
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) { m = umax32(m, __shfl_xor(m, x)); }
  if (lane_id() == 0) { s_max[threadIdx.x >> 6] = m; }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) { share_last[blockIdx.x] = umax32(umax32(s_max[0], s_max[1]), umax32(s_max[2], s_max[3])); }
}
// one workgroup, in place: share_last[b] becomes the largest mark IN FRONT of workgroup b's words
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_ann_carry(u32 *__restrict__ share_last, u32 shares) {
  __shared__ u32 s_part[QUERY_THREADS];
  const u32 per = (shares + QUERY_THREADS - 1u) / QUERY_THREADS;
  const u32 lo = min(threadIdx.x * per, shares), hi = min(lo + per, shares);
  u32 m = 0;
  for (u32 i = lo; i < hi; i++) { m = umax32(m, share_last[i]); }
  s_part[threadIdx.x] = m;
  lds_writes_done();
  __syncthreads();
  u32 run = 0;
  for (u32 t = 0; t < threadIdx.x; t++) { run = umax32(run, s_part[t]); }
  for (u32 i = lo; i < hi; i++) {
    const u32 x = share_last[i];
    share_last[i] = run;
    run = umax32(run, x);
  }
}
// head[i] and, in depth[i], the word's +1 / -1 / 0 (the scan behind this kernel makes it the depth); *scan_n = n
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_annotate(const u64 *__restrict__ tape, u32 n, const u32 *__restrict__ share_carry, u8 *__restrict__ head,
                                                               int *__restrict__ depth, u32 *__restrict__ scan_n) {
  __shared__ u32 s_wave[QUERY_THREADS / 64];
  const u64 i0 = u64(blockIdx.x) * WIDE_SHARE + u64(threadIdx.x) * WIDE_LANE_WORDS;
  u64 w[WIDE_LANE_WORDS];
  u32 mk[WIDE_LANE_WORDS], m = 0;
#pragma unroll
  for (u32 j = 0; j < WIDE_LANE_WORDS; j++) {
    w[j] = i0 + j < n ? tape[i0 + j] : 0;
    mk[j] = i0 + j < n ? wide_mark(w[j], i0 + j) : 0u;
    m = umax32(m, mk[j]);
  }
  u32 incl = m; // the running maximum over the lanes of the wave (a lane below the distance gets its own value back)
#pragma unroll
  for (u32 d = 1; d < 64; d <<= 1) { incl = umax32(incl, __shfl_up(incl, d)); }
  u32 run = __shfl_up(incl, 1u);
  if (lane_id() == 0) { run = 0; }
  if (lane_id() == 63) { s_wave[threadIdx.x >> 6] = incl; }
  lds_writes_done();
  __syncthreads();
  run = umax32(run, share_carry[blockIdx.x]);
  for (u32 v = 0; v < (threadIdx.x >> 6); v++) { run = umax32(run, s_wave[v]); }
  u32 heads = 0;
  int delta[WIDE_LANE_WORDS];
#pragma unroll
  for (u32 j = 0; j < WIDE_LANE_WORDS; j++) {
    const bool is_head = ((u32(i0 + j) - run) & 1u) == 0;
    const u32 t = u32(w[j] >> 56);
    delta[j] = !is_head ? 0 : (is_container_tag(t) ? 1 : ((t == '}' || t == ']') ? -1 : 0));
    heads |= (is_head ? 1u : 0u) << (8u * j);
    run = umax32(run, mk[j]);
  }
  if (i0 + WIDE_LANE_WORDS <= n) {
    *reinterpret_cast<u32 *>(head + i0) = heads;
    *reinterpret_cast<int4 *>(depth + i0) = make_int4(delta[0], delta[1], delta[2], delta[3]);
  } else {
#pragma unroll
    for (u32 j = 0; j < WIDE_LANE_WORDS; j++) {
      if (i0 + j < n) {
        head[i0 + j] = u8(heads >> (8u * j));
        depth[i0 + j] = delta[j];
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { *scan_n = n; }
}

// the starting frontier: the documents whose root is a container.  root[d] / flag[d] for d < docs, flag[docs] = 0, *scan_n = docs + 1
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_roots(const u64 *__restrict__ tape, const doc_span_dev *__restrict__ table, u32 docs, u32 *__restrict__ root,
                                                            int *__restrict__ flag, u32 *__restrict__ scan_n) {
  const u64 d64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (d64 > docs) { return; }
  const u32 d = u32(d64);
  if (d == docs) {
    flag[d] = 0;
    *scan_n = docs + 1u;
    return;
  }
  const u64 cur = u64(table[d].tape_begin) + 1u, doc_end = table[d + 1u].tape_begin;
  root[d] = u32(cur);
  flag[d] = cur < doc_end && is_container_tag(u32(tape[cur] >> 56)) ? 1 : 0;
}
// out[slot[e]] = src[e] for the entries whose flag was set (slot: the exclusive scan of the n + 1 flags)
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_compact(const u32 *__restrict__ src, const int *__restrict__ slot, u32 n, u32 *__restrict__ out) {
  const u64 e = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (e < n && slot[e + 1u] != slot[e]) { out[slot[e]] = src[e]; }
}
// level 0 is an ERR22: INVALID_JSON_POINTER for every container root
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_status(const doc_span_dev *__restrict__ table, u32 docs, const u32 *__restrict__ frontier, u32 F, u32 code,
                                                             u8 *__restrict__ status_row) {
  const u64 e = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (e < F) { status_row[wide_doc_of(table, docs, frontier[e])] = u8(code); }
}
// a PTR or TAIL level: one lane per element of the frontier.  found[e] / flag[e] for e < F, flag[F] = 0, *scan_n = F + 1; status_row (level 0 of a TAIL,
// else null): the code of an element that is a root
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_walk(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, const doc_span_dev *__restrict__ table, u32 docs,
                                                           const u8 *__restrict__ prog, u32 tokens_at, u32 keys_at, u32 k, u32 first_token, u32 n_tokens,
                                                           const u32 *__restrict__ frontier, u32 F, u8 *__restrict__ status_row, u32 *__restrict__ found, int *__restrict__ flag,
                                                           u32 *__restrict__ scan_n) {
  __shared__ query_token s_tok[PATH_MAX_TOKENS];
  __shared__ u64 s_key[QUERY_KEY_AREA / 8];
  const u32 tid = threadIdx.x;
  const path_header ph = reinterpret_cast<const path_header *>(prog)[k];
  {
    // the path's tokens and key area, as k_at_paths brings them in
    const u32 n_tok = ph.tokens < PATH_MAX_TOKENS ? ph.tokens : PATH_MAX_TOKENS;
    const u64 *src = reinterpret_cast<const u64 *>(prog + tokens_at) + u64(ph.first_token) * (sizeof(query_token) / 8);
    u64 *dst = reinterpret_cast<u64 *>(s_tok);
    for (u32 j = tid; j < n_tok * u32(sizeof(query_token) / 8); j += QUERY_THREADS) { dst[j] = src[j]; }
    u32 key_words = 0;
    if (n_tok) {
      const query_token last = reinterpret_cast<const query_token *>(prog + tokens_at)[ph.first_token + n_tok - 1u];
      key_words = (last.key_off + last.key_len + 7u) / 8u;
    }
    key_words = key_words < QUERY_KEY_AREA / 8 ? key_words : QUERY_KEY_AREA / 8;
    const u64 *ksrc = reinterpret_cast<const u64 *>(prog + keys_at + ph.keys_at);
    for (u32 j = tid; j < key_words; j += QUERY_THREADS) { s_key[j] = ksrc[j]; }
  }
  lds_writes_done();
  __syncthreads();
  const u64 e64 = u64(blockIdx.x) * QUERY_THREADS + tid;
  if (e64 > F) { return; }
  const u32 e = u32(e64);
  if (e == F) {
    flag[e] = 0;
    *scan_n = F + 1u;
    return;
  }
  u64 cur = frontier[e];
  u64 w = tape[cur];
  int ok = 0;
  if (is_container_tag(u32(w >> 56))) { // a scalar contributes nothing at any level, and is no error
    const u32 d = wide_doc_of(table, docs, u32(cur));
    const uint4 a = *reinterpret_cast<const uint4 *>(table + d), b = *reinterpret_cast<const uint4 *>(table + d + 1u);
    u64 limit = b.z; // the end of the document, and -- the frontier's elements lie side by side -- the next element: what is found stays in front of it, so every list ascends
    if (e + 1u < F) {
      const u64 next = frontier[e + 1u];
      limit = limit < next ? limit : next;
    }
    const u32 c = walk_tokens(tape, sbuf, s_tok + first_token, n_tokens, reinterpret_cast<const u8 *>(s_key), a.z, limit, a.w, b.w, cur, w);
    ok = c ? 0 : 1;
    if (c && status_row) { status_row[d] = u8(c); }
  }
  found[e] = u32(cur);
  flag[e] = ok;
}
// a WILD or WILD_LAST level, 1: ext[e] = the words between container e and its closing word (0 for a scalar) for e < F, ext[F] = 0, *scan_n = F + 1
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_extents(const u64 *__restrict__ tape, const doc_span_dev *__restrict__ table, u32 docs, const u32 *__restrict__ frontier,
                                                              u32 F, int *__restrict__ ext, u32 *__restrict__ scan_n) {
  const u64 e64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (e64 > F) { return; }
  const u32 e = u32(e64);
  if (e == F) {
    ext[e] = 0;
    *scan_n = F + 1u;
    return;
  }
  const u64 idx = frontier[e], w = tape[idx];
  u32 words = 0;
  if (is_container_tag(u32(w >> 56))) {
    const u32 d = wide_doc_of(table, docs, u32(idx));
    const u64 base = table[d].tape_begin, doc_end = table[d + 1u].tape_begin;
    u64 end = base + (w & LOW32);
    end = end > idx ? end - 1u : idx; // the closing word
    end = end < doc_end ? end : doc_end;
    if (e + 1u < F) { // the next element of the frontier lies behind this one's closing word
      const u64 next = frontier[e + 1u];
      end = end < next ? end : next;
    }
    words = end > idx + 1u ? u32(end - idx - 1u) : 0u;
  }
  ext[e] = int(words);
}
// 2: one lane per word of the range space (start: the scanned extents, R = start[F]): child[r] = the word begins a child of its container, child[R] = 0, *scan_n = R + 1
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_children(const u32 *__restrict__ frontier, u32 F, const u32 *__restrict__ start, u32 R, const u8 *__restrict__ head,
                                                               const int *__restrict__ depth, int *__restrict__ child, u32 *__restrict__ scan_n) {
  const u64 r64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (r64 > R) { return; }
  const u32 r = u32(r64);
  if (r == R) {
    child[r] = 0;
    *scan_n = R + 1u;
    return;
  }
  const u32 e = wide_parent_of(start, F, r);
  const u32 open = frontier[e], i = open + 1u + (r - start[e]);
  child[r] = head[i] && u32(depth[i]) - u32(depth[open]) == 1u ? 1 : 0;
}
// 3: values[e] = the child VALUES of container e (rank: the scanned child flags): an array's children, every second child of an object; values[F] = 0, *scan_n = F + 1
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_counts(const u64 *__restrict__ tape, const u32 *__restrict__ frontier, u32 F, const u32 *__restrict__ start,
                                                             const int *__restrict__ rank, int *__restrict__ values, u32 *__restrict__ scan_n) {
  const u64 e64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (e64 > F) { return; }
  const u32 e = u32(e64);
  if (e == F) {
    values[e] = 0;
    *scan_n = F + 1u;
    return;
  }
  const u32 children = u32(rank[start[e + 1u]]) - u32(rank[start[e]]);
  values[e] = int(u32(tape[frontier[e]] >> 56) == '{' ? children / 2u : children);
}
// 4: the child values in index order into out (first: the scanned counts): child j of an array is its value j, child 2 j + 1 of an object its value j (the even ones are the keys)
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_scatter(const u64 *__restrict__ tape, const u32 *__restrict__ frontier, u32 F, const u32 *__restrict__ start, u32 R,
                                                              const int *__restrict__ rank, const u32 *__restrict__ first, u32 *__restrict__ out) {
  const u64 r64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (r64 >= R) { return; }
  const u32 r = u32(r64);
  if (rank[r + 1u] == rank[r]) { return; }
  const u32 e = wide_parent_of(start, F, r);
  const u32 open = frontier[e], j = u32(rank[r]) - u32(rank[start[e]]);
  u32 at = j;
  if (u32(tape[open] >> 56) == '{') {
    if ((j & 1u) == 0) { return; }
    at = j / 2u;
  }
  if (first[e] + at < first[e + 1u]) { out[first[e] + at] = open + 1u + (r - start[e]); }
}
// the cells of one path: its matches are one ascending list, the cell of document d the slice of the indices in [tape_begin[d], tape_begin[d + 1]).
// offsets_row[d] = running + the matches in front of document d; with_total: offsets_row[docs] = running + count (the last path's: the column's total)
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_offsets(const doc_span_dev *__restrict__ table, u32 docs, const u32 *__restrict__ list, u32 count, u32 running,
                                                              u32 with_total, u32 *__restrict__ offsets_row) {
  const u64 d64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (d64 > docs || (d64 == docs && !with_total)) { return; }
  u32 lo = 0, hi = count; // the first match at or behind tape_begin[d]
  if (d64 < docs) {
    const u32 begin = table[d64].tape_begin;
    while (lo < hi) {
      const u32 mid = lo + (hi - lo) / 2u;
      if (list[mid] < begin) { lo = mid + 1u; } else { hi = mid; }
    }
  }
  offsets_row[d64] = running + hi;
}
// one lane per match: value / tag begin at the path's first match
__global__ __launch_bounds__(QUERY_THREADS) void k_wide_emit(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, const doc_span_dev *__restrict__ table, u32 docs,
                                                           const u32 *__restrict__ list, u32 count, u64 *__restrict__ value, u8 *__restrict__ tag) {
  const u64 j = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (j >= count) { return; }
  const u64 cur = list[j], w = tape[cur];
  const u32 d = wide_doc_of(table, docs, u32(cur));
  const uint4 a = *reinterpret_cast<const uint4 *>(table + d), b = *reinterpret_cast<const uint4 *>(table + d + 1u);
  tag[j] = u8(w >> 56);
  value[j] = cell_value(tape, sbuf, cur, w, a.z, b.z, a.w, b.w);
}

// ---- the rows (include/sjgpu_rows.h: sjgpu_at_pointers_from_cells_device) ---------------------------------------------------------------------------
// at_pointer of K pointers rooted at the CELLS of one row: K x rows cells, one lane each, mapped like k_at_pointers.  What a root is -- its document, or
// that no walk is needed -- does not depend on the pointer, so it is settled once per root by k_rows_locate and left in 4 bytes:
//   below ROWS_SPECIAL           the document d of a container root whose cell agrees with the tape
//   ROWS_SPECIAL                 a scalar root: the empty pointer copies the cell, any other gets the scalar's verdict from the program
//   ROWS_SPECIAL | (code - 16)   every pointer answers `code` (a failed root keeps its 17 / 19 / 20 / 22; a tag that is none, or a container cell that disagrees
//                                with the tape, is NO_SUCH_FIELD)
// (docs is below 0xFFFFFFF0: the C-ABI refuses more.)
// (ROWS_SPECIAL and rows_code: sjgpu_internal.h -- sjgpu_json.hip reads the same verdicts)

__device__ __forceinline__ bool is_query_code(u32 t) {
  return t == QUERY_INCORRECT_TYPE || t == QUERY_INDEX_OUT_OF_BOUNDS || t == QUERY_NO_SUCH_FIELD || t == QUERY_INVALID_JSON_POINTER;
}

// one lane per root.  A container cell is followed only when its opening index c lies INSIDE a document (behind its root word), the word there carries the
// cell's tag and points where the cell's high half says: log2(docs) table reads, one tape word.
__global__ __launch_bounds__(QUERY_THREADS) void k_rows_locate(const u64 *__restrict__ tape, const doc_span_dev *__restrict__ table, u32 docs, const u64 *__restrict__ root_value,
                                                             const u8 *__restrict__ root_tag, u32 rows, u32 *__restrict__ where) {
  const u64 r64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (r64 >= rows) { return; }
  const u32 t = root_tag[r64];
  u32 out = ROWS_SPECIAL | (QUERY_NO_SUCH_FIELD - 16u);
  if (is_container_tag(t)) {
    const u64 v = root_value[r64];
    const u32 c = u32(v & LOW32);
    if (docs && c > table[0].tape_begin) {
      const u32 d = wide_doc_of(table, docs, c);
      const u64 base = table[d].tape_begin, doc_end = table[d + 1u].tape_begin;
      if (c > base && c < doc_end) { // (at or behind the last entry: outside every document)
        const u64 w = tape[c];
        if (u32(w >> 56) == t && base + (w & LOW32) == (v >> 32)) { out = d; }
      }
    }
  } else if (t == '"' || is_number_tag(t) || t == 't' || t == 'f' || t == 'n') {
    out = ROWS_SPECIAL;
  } else if (is_query_code(t)) {
    out = ROWS_SPECIAL | (t - 16u);
  }
  where[r64] = out;
}

// grid: K rows of row_blocks workgroups, row k = pointer k; lane = root
__global__ __launch_bounds__(QUERY_THREADS) void k_at_pointers_rooted(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, const doc_span_dev *__restrict__ table,
                                                                    const u64 *__restrict__ root_value, const u8 *__restrict__ root_tag, const u32 *__restrict__ where, u32 rows,
                                                                    const u8 *__restrict__ prog, u32 tokens_at, u32 keys_at, u32 row_blocks, u64 *__restrict__ value,
                                                                    u8 *__restrict__ tag) {
  __shared__ query_token s_tok[QUERY_MAX_TOKENS];
  __shared__ u64 s_key[QUERY_KEY_AREA / 8];
  const u32 k = blockIdx.x / row_blocks, row_block = blockIdx.x - k * row_blocks;
  const query_pointer qp = reinterpret_cast<const query_pointer *>(prog)[k];
  stage_pointer(prog, tokens_at, keys_at, qp, s_tok, s_key);
  const u64 r64 = u64(row_block) * QUERY_THREADS + threadIdx.x;
  if (r64 >= rows) { return; }
  const u32 m = where[r64];
  u32 out_tag;
  u64 out_value = 0;
  if (m > ROWS_SPECIAL) {
    out_tag = rows_code(m);
  } else if (m == ROWS_SPECIAL) {
    if (qp.code) {
      out_tag = qp.code;
    } else if (qp.tokens) {
      out_tag = s_tok[0].scalar_code;
    } else {
      out_tag = root_tag[r64];
      out_value = root_value[r64];
    }
  } else {
    const uint4 a = *reinterpret_cast<const uint4 *>(table + m), b = *reinterpret_cast<const uint4 *>(table + m + 1u);
    const u64 base = a.z, doc_end = b.z;
    const u64 str_base = a.w, str_end = b.w;
    u32 code = qp.code;
    if (!code) {
      const u64 v = root_value[r64];
      u64 cur = v & LOW32, w = tape[cur]; // (k_rows_locate found cur inside the document, and w to agree with the cell)
      const u64 limit = (v >> 32) < doc_end ? (v >> 32) : doc_end;
      code = walk_tokens(tape, sbuf, s_tok, qp.tokens, reinterpret_cast<const u8 *>(s_key), base, limit, str_base, str_end, cur, w);
      if (!code) { out_value = cell_value(tape, sbuf, cur, w, base, doc_end, str_base, str_end); }
      out_tag = code ? code : u32(w >> 56);
    } else {
      out_tag = code;
    }
  }
  const u64 cell = u64(k) * rows + r64;
  tag[cell] = u8(out_tag);
  value[cell] = out_value;
}

// ---- the lists (include/sjgpu_lists.h: sjgpu_at_paths_from_cells_device) ----------------------------------------------------------------------------
// at_path_with_wildcard of K paths rooted at the CELLS of one row: K x rows cells, one lane each, mapped and counted / scanned / filled like k_at_paths.  What a
// root is comes from k_rows_locate, once per call for all K paths and both passes: a located container walks from its opening word, bounded by the cell's high
// half cut to its document's end; a scalar root is status 0 without a match; everything else its code (a disagreeing cell: 20) without a match -- whatever the path.
// grid: K rows of row_blocks workgroups, row k = path k; lane = root
template <bool FILL>
__global__ __launch_bounds__(QUERY_THREADS) void k_at_paths_rooted(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, const doc_span_dev *__restrict__ table,
                                                                 const u64 *__restrict__ root_value, const u32 *__restrict__ where, u32 rows, const u8 *__restrict__ prog,
                                                                 u32 levels_at, u32 tokens_at, u32 keys_at, u32 row_blocks, u32 *__restrict__ offsets, u8 *__restrict__ status,
                                                                 u64 *__restrict__ block_sums, u64 *__restrict__ value, u8 *__restrict__ tag) {
  __shared__ query_token s_tok[PATH_MAX_TOKENS];
  __shared__ u64 s_key[QUERY_KEY_AREA / 8];
  __shared__ path_level s_lev[PATH_MAX_LEVELS];
  __shared__ u32 s_cur[PATH_MAX_WILDS][QUERY_THREADS], s_end[PATH_MAX_WILDS][QUERY_THREADS];
  __shared__ u64 s_sum[QUERY_THREADS / 64];
  const u32 k = blockIdx.x / row_blocks, row_block = blockIdx.x - k * row_blocks, tid = threadIdx.x;
  const path_header ph = reinterpret_cast<const path_header *>(prog)[k];
  stage_path(prog, levels_at, tokens_at, keys_at, ph, s_lev, s_tok, s_key);
  const u64 r64 = u64(row_block) * QUERY_THREADS + tid;
  const bool active = r64 < rows;
  const u64 cell = u64(k) * rows + r64;
  u32 count = 0, code = 0;
  u64 out = 0, out_end = 0; // FILL: the cell's matches are value / tag[out .. out_end)
  bool go = active;
  if (FILL && active) {
    out = offsets[cell];
    out_end = offsets[cell + 1u];
    go = out < out_end; // (a cell without matches, or with a status, has nothing to write)
  }
  if (go) {
    const u32 m = where[r64];
    if (m > ROWS_SPECIAL) {
      code = rows_code(m);
    } else if (m < ROWS_SPECIAL) { // (ROWS_SPECIAL itself: a scalar, status 0 and nothing)
      const uint4 a = *reinterpret_cast<const uint4 *>(table + m), b = *reinterpret_cast<const uint4 *>(table + m + 1u);
      const u64 base = a.z, doc_end = b.z;
      const u64 str_base = a.w, str_end = b.w;
      const u64 v = root_value[r64];
      const u64 cur = v & LOW32, w = tape[cur]; // (k_rows_locate found cur inside the document, and w to agree with the cell)
      const u64 outer = (v >> 32) < doc_end ? (v >> 32) : doc_end;
      walk_levels<FILL>(tape, sbuf, s_lev, ph.levels, s_tok, reinterpret_cast<const u8 *>(s_key), s_cur, s_end, cur, w, outer, base, doc_end, str_base, str_end, count, code, out,
                        out_end, value, tag);
    }
  }
  if (FILL) { return; }
  paths_count_done(active, cell, count, code, rows, row_blocks, offsets, status, block_sums, s_sum);
}

// ---- the fields (include/sjgpu_fields.h: sjgpu_object_fields_from_cells_device, sjgpu_cell_sizes_device) --------------------------------------------------
// `for (dom::key_value_pair f : dom::object(e))` of every root cell of one row: the fields of each cell's object as one ragged pair of rows, keys as string cells and
// values as cells, counted / scanned / filled like the lists -- one lane per root, consecutive lanes consecutive roots, k_rows_locate's verdicts.  No path, no
// program, no key area.  The count does NOT walk: an opening word carries its scope's count in bits 32 .. 55 (the reference's tape_ref::scope_count), saturated at
// 0xFFFFFF; only a count that reads saturated is walked.  The fill walks once and never trusts the count: it stops at the cell's last slot and pads what it did not reach.
constexpr u32 SCOPE_COUNT_SATURATED = 0xFFFFFFu;
__device__ __forceinline__ u32 scope_count(u64 w) { return u32(w >> 32) & SCOPE_COUNT_SATURATED; }

// the fields of the object that opens at word `cur` (its word: w), in the tape's order; outer: the end of what surrounds it (the cell's high half cut to the
// document's end).  FILL: field j to the four rows at out + j while out + j < out_end, and the slots behind the last field, up to out_end, padded with
// NO_SUCH_FIELD and zeros; else the fields are counted.  -> the count
template <bool FILL>
__device__ __forceinline__ u32 walk_fields(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 cur, u64 w, u64 outer, u64 base, u64 doc_end, u64 str_base, u64 str_end,
                                           u64 out, u64 out_end, u64 *__restrict__ key_value, u8 *__restrict__ key_tag, u64 *__restrict__ value, u8 *__restrict__ tag) {
  u64 end = base + (w & LOW32);
  end = end > cur ? end - 1u : cur; // the closing word
  end = end < outer ? end : outer;
  u64 i = cur + 1u; // the first key
  u32 count = 0;
  while (i + 1u < end && (!FILL || out < out_end)) { // a key word and the first word of its value
    const u64 vw = tape[i + 1u];
    if (FILL) {
      key_tag[out] = u8('"');
      key_value[out] = string_cell_value(sbuf, tape[i], str_base, str_end);
      tag[out] = u8(vw >> 56);
      value[out] = cell_value(tape, sbuf, i + 1u, vw, base, doc_end, str_base, str_end);
      out++;
    }
    count++;
    i = behind(i + 1u, vw, base, end);
  }
  if (FILL) {
    for (; out < out_end; out++) { // (a count field that claims more than the walk finds)
      key_tag[out] = u8(QUERY_NO_SUCH_FIELD);
      key_value[out] = 0;
      tag[out] = u8(QUERY_NO_SUCH_FIELD);
      value[out] = 0;
    }
  }
  return count;
}

// grid: ceil(rows / 256) workgroups; lane = root.  status: 0 for a located object, INCORRECT_TYPE for a located array and for a scalar, else the verdict's code
__global__ __launch_bounds__(QUERY_THREADS) void k_object_fields_count(const u64 *__restrict__ tape, const doc_span_dev *__restrict__ table, const u64 *__restrict__ root_value,
                                                                     const u32 *__restrict__ where, u32 rows, u32 *__restrict__ offsets, u8 *__restrict__ status,
                                                                     u64 *__restrict__ block_sums) {
  __shared__ u64 s_sum[QUERY_THREADS / 64];
  const u64 r64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  const bool active = r64 < rows;
  u32 count = 0, code = 0;
  if (active) {
    const u32 m = where[r64];
    if (m > ROWS_SPECIAL) {
      code = rows_code(m);
    } else if (m == ROWS_SPECIAL) {
      code = QUERY_INCORRECT_TYPE;
    } else {
      const u64 v = root_value[r64];
      const u64 cur = v & LOW32, w = tape[cur]; // (k_rows_locate found cur inside the document, and w to agree with the cell)
      if (u32(w >> 56) != '{') {
        code = QUERY_INCORRECT_TYPE;
      } else {
        count = scope_count(w);
        if (count == SCOPE_COUNT_SATURATED) { // 16 777 215 fields or more: the one case that is walked
          const u64 base = table[m].tape_begin, doc_end = table[m + 1u].tape_begin;
          const u64 outer = (v >> 32) < doc_end ? (v >> 32) : doc_end;
          count = walk_fields<false>(tape, nullptr, cur, w, outer, base, doc_end, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr);
        }
      }
    }
  }
  paths_count_done(active, r64, count, code, rows, gridDim.x, offsets, status, block_sums, s_sum);
}

// grid: ceil(rows / 256) workgroups; lane = root.  The slots of root r are offsets[r] .. offsets[r + 1]: only a located object has any
__global__ __launch_bounds__(QUERY_THREADS) void k_object_fields_fill(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, const doc_span_dev *__restrict__ table,
                                                                    const u64 *__restrict__ root_value, const u32 *__restrict__ where, u32 rows,
                                                                    const u32 *__restrict__ offsets, u64 *__restrict__ key_value, u8 *__restrict__ key_tag,
                                                                    u64 *__restrict__ value, u8 *__restrict__ tag) {
  const u64 r64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (r64 >= rows) { return; }
  const u64 out = offsets[r64], out_end = offsets[r64 + 1u];
  if (out >= out_end) { return; }
  const u32 m = where[r64];
  if (m >= ROWS_SPECIAL) { return; } // (the count gave such a root no slot)
  const uint4 a = *reinterpret_cast<const uint4 *>(table + m), b = *reinterpret_cast<const uint4 *>(table + m + 1u);
  const u64 base = a.z, doc_end = b.z;
  const u64 str_base = a.w, str_end = b.w;
  const u64 v = root_value[r64];
  const u64 cur = v & LOW32, w = tape[cur];
  const u64 outer = (v >> 32) < doc_end ? (v >> 32) : doc_end;
  walk_fields<true>(tape, sbuf, cur, w, outer, base, doc_end, str_base, str_end, out, out_end, key_value, key_tag, value, tag);
}

// dom::object::size() / dom::array::size() of every root: the count field of a located container's opening word as it stands, no walk.  lane = root
__global__ __launch_bounds__(QUERY_THREADS) void k_cell_sizes(const u64 *__restrict__ tape, const u64 *__restrict__ root_value, const u32 *__restrict__ where, u32 rows,
                                                            u32 *__restrict__ size, u8 *__restrict__ code_out) {
  const u64 r64 = u64(blockIdx.x) * QUERY_THREADS + threadIdx.x;
  if (r64 >= rows) { return; }
  const u32 m = where[r64];
  u32 n = 0, code = 0;
  if (m > ROWS_SPECIAL) {
    code = rows_code(m);
  } else if (m == ROWS_SPECIAL) {
    code = QUERY_INCORRECT_TYPE;
  } else {
    n = scope_count(tape[root_value[r64] & LOW32]);
  }
  size[r64] = n;
  code_out[r64] = u8(code);
}

static inline u32 blocks_of(u64 n, u32 per) { return u32((n + per - 1) / per); }

} // namespace

void launch_query_check_table(const doc_span_dev *table, uint32_t docs, uint64_t tape_words, uint64_t string_bytes, uint32_t *bad, hipStream_t s) {
  hipLaunchKernelGGL(k_query_check_table, dim3(blocks_of(u64(docs) + 1, QUERY_THREADS)), dim3(QUERY_THREADS), 0, s, table, docs, tape_words, string_bytes, bad);
}

void launch_at_pointers(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint8_t *program, uint32_t tokens_at,
                        uint32_t keys_at, uint32_t K, uint64_t *value, uint8_t *tag, hipStream_t s) {
  const u32 row_blocks = blocks_of(docs, QUERY_THREADS);
  hipLaunchKernelGGL(k_at_pointers, dim3(row_blocks * K), dim3(QUERY_THREADS), 0, s, tape, string_buf, table, docs, program, tokens_at, keys_at, row_blocks, value, tag);
}

void launch_at_pointers_rooted(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag,
                               uint32_t rows, uint32_t *where, const uint8_t *program, uint32_t tokens_at, uint32_t keys_at, uint32_t K, uint64_t *value, uint8_t *tag,
                               hipStream_t s) {
  const u32 row_blocks = blocks_of(rows, QUERY_THREADS);
  hipLaunchKernelGGL(k_rows_locate, dim3(row_blocks), dim3(QUERY_THREADS), 0, s, tape, table, docs, root_value, root_tag, rows, where);
  hipLaunchKernelGGL(k_at_pointers_rooted, dim3(row_blocks * K), dim3(QUERY_THREADS), 0, s, tape, string_buf, table, root_value, root_tag, where, rows, program, tokens_at, keys_at,
                     row_blocks, value, tag);
}

// [ctrl, 256 bytes][the blocks' sums][the scan's block sums]
static inline size_t gather_sums_bytes(uint32_t docs) { return (size_t(blocks_of(u64(docs) + 1, GATHER_BLOCK)) * sizeof(u64) + 255) & ~size_t(255); }
size_t gather_workspace_bytes(uint32_t docs) { return 256 + gather_sums_bytes(docs) + (size_t(blocks_of(u64(docs) + 1, 4096)) + 64) * sizeof(int); }

const void *launch_gather_offsets(const uint64_t *value, const uint8_t *tag, uint32_t docs, uint64_t string_bytes, uint32_t *offsets, void *workspace, hipStream_t s) {
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  gather_ctrl *ctrl = reinterpret_cast<gather_ctrl *>(ws);
  u64 *block_sums = reinterpret_cast<u64 *>(ws + 256);
  int *partial = reinterpret_cast<int *>(ws + 256 + gather_sums_bytes(docs));
  const u32 blocks = blocks_of(u64(docs) + 1, GATHER_BLOCK);
  hipLaunchKernelGGL(k_gather_lengths, dim3(blocks), dim3(QUERY_THREADS), 0, s, value, tag, docs, string_bytes, offsets, block_sums);
  hipLaunchKernelGGL(k_gather_total, dim3(1), dim3(QUERY_THREADS), 0, s, block_sums, blocks, docs, ctrl);
  enqueue_scan(reinterpret_cast<int *>(offsets), docs + 1u, &ctrl->n_plus_1, partial, s);
  return ctrl;
}

void launch_gather_copy(const uint8_t *string_buf, const uint64_t *value, const uint32_t *offsets, uint32_t docs, uint64_t total, uint8_t *chars, hipStream_t s) {
  if (total == 0 || docs == 0) { return; }
  hipLaunchKernelGGL(k_gather_copy, dim3(blocks_of(total, QUERY_THREADS * GATHER_CHUNK)), dim3(QUERY_THREADS), 0, s, string_buf, value, offsets, docs, total, chars);
}

// [ctrl, 256 bytes][the count kernel's block sums][the scan's block sums]
static inline size_t paths_sums_bytes(uint32_t K, uint32_t docs) { return (size_t(blocks_of(docs, QUERY_THREADS)) * K * sizeof(u64) + 255) & ~size_t(255); }
size_t paths_workspace_bytes(uint32_t K, uint32_t docs) { return 256 + paths_sums_bytes(K, docs) + (size_t(blocks_of(u64(K) * docs + 1, 4096)) + 64) * sizeof(int); }

const void *launch_paths_count(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint8_t *program, uint32_t levels_at,
                               uint32_t tokens_at, uint32_t keys_at, uint32_t K, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s) {
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  gather_ctrl *ctrl = reinterpret_cast<gather_ctrl *>(ws);
  u64 *block_sums = reinterpret_cast<u64 *>(ws + 256);
  int *partial = reinterpret_cast<int *>(ws + 256 + paths_sums_bytes(K, docs));
  const u32 row_blocks = blocks_of(docs, QUERY_THREADS), cells = K * docs;
  hipLaunchKernelGGL(k_at_paths<false>, dim3(row_blocks * K), dim3(QUERY_THREADS), 0, s, tape, string_buf, table, docs, program, levels_at, tokens_at, keys_at, row_blocks, offsets,
                     status, block_sums, static_cast<u64 *>(nullptr), static_cast<u8 *>(nullptr));
  hipLaunchKernelGGL(k_gather_total, dim3(1), dim3(QUERY_THREADS), 0, s, block_sums, row_blocks * K, cells, ctrl);
  enqueue_scan(reinterpret_cast<int *>(offsets), cells + 1u, &ctrl->n_plus_1, partial, s);
  return ctrl;
}

void launch_paths_fill(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint8_t *program, uint32_t levels_at, uint32_t tokens_at,
                       uint32_t keys_at, uint32_t K, const uint32_t *offsets, uint64_t *value, uint8_t *tag, hipStream_t s) {
  const u32 row_blocks = blocks_of(docs, QUERY_THREADS);
  hipLaunchKernelGGL(k_at_paths<true>, dim3(row_blocks * K), dim3(QUERY_THREADS), 0, s, tape, string_buf, table, docs, program, levels_at, tokens_at, keys_at, row_blocks,
                     const_cast<u32 *>(offsets), static_cast<u8 *>(nullptr), static_cast<u64 *>(nullptr), value, tag);
}

// the same count and fill rooted at the cells of one row (include/sjgpu_lists.h); where[0 .. rows): k_rows_locate's verdicts, made here in front of the count
const void *launch_paths_rooted_count(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value,
                                      const uint8_t *root_tag, uint32_t rows, uint32_t *where, const uint8_t *program, uint32_t levels_at, uint32_t tokens_at, uint32_t keys_at,
                                      uint32_t K, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s) {
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  gather_ctrl *ctrl = reinterpret_cast<gather_ctrl *>(ws);
  u64 *block_sums = reinterpret_cast<u64 *>(ws + 256);
  int *partial = reinterpret_cast<int *>(ws + 256 + paths_sums_bytes(K, rows));
  const u32 row_blocks = blocks_of(rows, QUERY_THREADS), cells = K * rows;
  hipLaunchKernelGGL(k_rows_locate, dim3(row_blocks), dim3(QUERY_THREADS), 0, s, tape, table, docs, root_value, root_tag, rows, where);
  hipLaunchKernelGGL(k_at_paths_rooted<false>, dim3(row_blocks * K), dim3(QUERY_THREADS), 0, s, tape, string_buf, table, root_value, static_cast<const u32 *>(where), rows, program,
                     levels_at, tokens_at, keys_at, row_blocks, offsets, status, block_sums, static_cast<u64 *>(nullptr), static_cast<u8 *>(nullptr));
  hipLaunchKernelGGL(k_gather_total, dim3(1), dim3(QUERY_THREADS), 0, s, block_sums, row_blocks * K, cells, ctrl);
  enqueue_scan(reinterpret_cast<int *>(offsets), cells + 1u, &ctrl->n_plus_1, partial, s);
  return ctrl;
}

void launch_paths_rooted_fill(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, const uint64_t *root_value, uint32_t rows, const uint32_t *where,
                              const uint8_t *program, uint32_t levels_at, uint32_t tokens_at, uint32_t keys_at, uint32_t K, const uint32_t *offsets, uint64_t *value, uint8_t *tag,
                              hipStream_t s) {
  const u32 row_blocks = blocks_of(rows, QUERY_THREADS);
  hipLaunchKernelGGL(k_at_paths_rooted<true>, dim3(row_blocks * K), dim3(QUERY_THREADS), 0, s, tape, string_buf, table, root_value, where, rows, program, levels_at, tokens_at,
                     keys_at, row_blocks, const_cast<u32 *>(offsets), static_cast<u8 *>(nullptr), static_cast<u64 *>(nullptr), value, tag);
}

// the fields of the roots' objects (include/sjgpu_fields.h): locate, count, the total, the scan -- the workspace and the control block of one rooted path
const void *launch_object_fields_count(const uint64_t *tape, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag, uint32_t rows,
                                       uint32_t *where, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s) {
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  gather_ctrl *ctrl = reinterpret_cast<gather_ctrl *>(ws);
  u64 *block_sums = reinterpret_cast<u64 *>(ws + 256);
  int *partial = reinterpret_cast<int *>(ws + 256 + paths_sums_bytes(1, rows));
  const u32 row_blocks = blocks_of(rows, QUERY_THREADS);
  hipLaunchKernelGGL(k_rows_locate, dim3(row_blocks), dim3(QUERY_THREADS), 0, s, tape, table, docs, root_value, root_tag, rows, where);
  hipLaunchKernelGGL(k_object_fields_count, dim3(row_blocks), dim3(QUERY_THREADS), 0, s, tape, table, root_value, static_cast<const u32 *>(where), rows, offsets, status, block_sums);
  hipLaunchKernelGGL(k_gather_total, dim3(1), dim3(QUERY_THREADS), 0, s, block_sums, row_blocks, rows, ctrl);
  enqueue_scan(reinterpret_cast<int *>(offsets), rows + 1u, &ctrl->n_plus_1, partial, s);
  return ctrl;
}

void launch_object_fields_fill(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, const uint64_t *root_value, uint32_t rows, const uint32_t *where,
                               const uint32_t *offsets, uint64_t *key_value, uint8_t *key_tag, uint64_t *value, uint8_t *tag, hipStream_t s) {
  hipLaunchKernelGGL(k_object_fields_fill, dim3(blocks_of(rows, QUERY_THREADS)), dim3(QUERY_THREADS), 0, s, tape, string_buf, table, root_value, where, rows, offsets, key_value,
                     key_tag, value, tag);
}

// what the units beside this one share of it (sjgpu_json.hip): the roots' verdicts, and the 64-bit total of a count kernel's block sums with the scan's length
void launch_rows_locate(const uint64_t *tape, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag, uint32_t rows, uint32_t *where,
                        hipStream_t s) {
  hipLaunchKernelGGL(k_rows_locate, dim3(blocks_of(rows, QUERY_THREADS)), dim3(QUERY_THREADS), 0, s, tape, table, docs, root_value, root_tag, rows, where);
}

void launch_count_total(const uint64_t *block_sums, uint32_t blocks, uint32_t entries, count_total_dev *ctrl, hipStream_t s) {
  static_assert(sizeof(count_total_dev) == sizeof(gather_ctrl), "one control block");
  hipLaunchKernelGGL(k_gather_total, dim3(1), dim3(QUERY_THREADS), 0, s, block_sums, blocks, entries, reinterpret_cast<gather_ctrl *>(ctrl));
}

void launch_cell_sizes(const uint64_t *tape, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag, uint32_t rows, uint32_t *where,
                       uint32_t *size, uint8_t *code, hipStream_t s) {
  const u32 row_blocks = blocks_of(rows, QUERY_THREADS);
  hipLaunchKernelGGL(k_rows_locate, dim3(row_blocks), dim3(QUERY_THREADS), 0, s, tape, table, docs, root_value, root_tag, rows, where);
  hipLaunchKernelGGL(k_cell_sizes, dim3(row_blocks), dim3(QUERY_THREADS), 0, s, tape, root_value, static_cast<const u32 *>(where), rows, size, code);
}

// ---- the wide call's level loop ---------------------------------------------------------------------------------------------------------------------
namespace {
// [ctrl, 256 bytes][head: 1 byte per word][depth: 4][two frontiers: 4 + 4][extents, child flags / ranks, counts: 4 + 4 + 4 per entry][the annotation's
// workgroup marks][the roots: 4 per document][the scans' block sums]; entries: the larger of tape_words and docs, plus 1
struct wide_workspace {
  u32 *ctrl;
  u8 *head;
  int *depth;
  u32 *frontier[2];
  int *ext, *rank, *count;
  u32 *share, *roots;
  int *partial;
  size_t bytes;
};
wide_workspace carve_wide_workspace(void *base, uint32_t docs, uint64_t tape_words) {
  const size_t entries = size_t(tape_words > docs ? tape_words : docs) + 1;
  const uintptr_t p = reinterpret_cast<uintptr_t>(base); // (null when only the size is asked for)
  size_t at = 0;
  auto take = [&](size_t n) {
    uint8_t *q = reinterpret_cast<uint8_t *>(p + at);
    at += (n + 255) & ~size_t(255);
    return q;
  };
  wide_workspace w;
  w.ctrl = reinterpret_cast<u32 *>(take(256));
  w.head = take(size_t(tape_words));
  w.depth = reinterpret_cast<int *>(take(size_t(tape_words) * 4));
  w.frontier[0] = reinterpret_cast<u32 *>(take(size_t(tape_words) * 4));
  w.frontier[1] = reinterpret_cast<u32 *>(take(size_t(tape_words) * 4));
  w.ext = reinterpret_cast<int *>(take(entries * 4));
  w.rank = reinterpret_cast<int *>(take(entries * 4));
  w.count = reinterpret_cast<int *>(take(entries * 4));
  w.share = reinterpret_cast<u32 *>(take(size_t(blocks_of(tape_words, WIDE_SHARE)) * 4));
  w.roots = reinterpret_cast<u32 *>(take(size_t(docs) * 4));
  w.partial = reinterpret_cast<int *>(take((size_t(blocks_of(entries, 4096)) + 64) * 4));
  w.bytes = at;
  return w;
}
} // namespace

size_t paths_wide_workspace_bytes(uint32_t K, uint32_t docs, uint64_t tape_words) {
  (void)K; // the paths run one behind the other in the same blocks
  return carve_wide_workspace(nullptr, docs, tape_words).bytes;
}

#define WIDE_TRY(call)                     \
  do {                                     \
    const hipError_t e_ = (call);          \
    if (e_ != hipSuccess) { return e_; }   \
  } while (0)

hipError_t launch_paths_wide(const uint64_t *tape, uint64_t tape_words, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint8_t *program,
                             const uint8_t *program_host, uint32_t levels_at, uint32_t tokens_at, uint32_t keys_at, uint32_t K, uint32_t *offsets, uint8_t *status,
                             uint64_t *value, uint8_t *tag, uint64_t match_cap, void *workspace, uint32_t *readback, hipStream_t s, uint64_t *matches_out) {
  const wide_workspace W = carve_wide_workspace(workspace, docs, tape_words);
  const u32 n = u32(tape_words);
  const path_header *heads = reinterpret_cast<const path_header *>(program_host);
  const path_level *levels = reinterpret_cast<const path_level *>(program_host + levels_at);
  const dim3 T(QUERY_THREADS);
  // a frontier's size, a range space's size: four bytes the host waits for
  auto read_back = [&](const void *dev, u32 *out) -> hipError_t {
    WIDE_TRY(hipGetLastError());
    WIDE_TRY(hipMemcpyAsync(readback, dev, sizeof(u32), hipMemcpyDeviceToHost, s));
    WIDE_TRY(hipStreamSynchronize(s));
    *out = *readback;
    return hipSuccess;
  };
  auto scan = [&](int *a, u32 entries) { enqueue_scan(a, entries, W.ctrl, W.partial, s); }; // (the kernel in front of it left `entries` in ctrl[0])
  // the annotation, once for all paths
  if (n) {
    const u32 shares = blocks_of(n, WIDE_SHARE);
    hipLaunchKernelGGL(k_wide_ann_summary, dim3(shares), T, 0, s, tape, n, W.share);
    hipLaunchKernelGGL(k_wide_ann_carry, dim3(1), T, 0, s, W.share, shares);
    hipLaunchKernelGGL(k_wide_annotate, dim3(shares), T, 0, s, tape, n, W.share, W.head, W.depth, W.ctrl);
    scan(W.depth, n);
  }
  // the starting frontier, the same for every path
  u32 n_roots = 0;
  hipLaunchKernelGGL(k_wide_roots, dim3(blocks_of(u64(docs) + 1, QUERY_THREADS)), T, 0, s, tape, table, docs, reinterpret_cast<u32 *>(W.count), W.rank, W.ctrl);
  scan(W.rank, docs + 1u);
  hipLaunchKernelGGL(k_wide_compact, dim3(blocks_of(docs, QUERY_THREADS)), T, 0, s, reinterpret_cast<const u32 *>(W.count), W.rank, docs, W.roots);
  WIDE_TRY(read_back(W.rank + docs, &n_roots));

  // the levels of path k over all documents -> its matches, an ascending list in one of the frontier blocks.  first_run: the run that leaves the statuses
  auto run_levels = [&](u32 k, bool first_run, const u32 **list, u32 *count) -> hipError_t {
    const path_header &ph = heads[k];
    const u32 *cur = W.roots;
    u32 F = n_roots, flip = 0;
    *list = cur;
    *count = 0;
    for (u32 L = 0; L < ph.levels && F; L++) {
      const path_level &lv = levels[ph.first_level + L];
      u8 *status_row = first_run && L == 0 ? status + size_t(k) * docs : nullptr;
      u32 *out = W.frontier[flip];
      u32 next = 0;
      if (lv.kind == PATH_PTR || lv.kind == PATH_TAIL) {
        hipLaunchKernelGGL(k_wide_walk, dim3(blocks_of(u64(F) + 1, QUERY_THREADS)), T, 0, s, tape, string_buf, table, docs, program, tokens_at, keys_at, k, lv.first_token, lv.tokens,
                           cur, F, lv.kind == PATH_TAIL ? status_row : static_cast<u8 *>(nullptr), reinterpret_cast<u32 *>(W.count), W.rank, W.ctrl);
        scan(W.rank, F + 1u);
        hipLaunchKernelGGL(k_wide_compact, dim3(blocks_of(F, QUERY_THREADS)), T, 0, s, reinterpret_cast<const u32 *>(W.count), W.rank, F, out);
        WIDE_TRY(read_back(W.rank + F, &next));
      } else if (lv.kind == PATH_WILD || lv.kind == PATH_WILD_LAST) {
        u32 R = 0;
        const u32 *start = reinterpret_cast<const u32 *>(W.ext);
        hipLaunchKernelGGL(k_wide_extents, dim3(blocks_of(u64(F) + 1, QUERY_THREADS)), T, 0, s, tape, table, docs, cur, F, W.ext, W.ctrl);
        scan(W.ext, F + 1u);
        WIDE_TRY(read_back(W.ext + F, &R));
        if (R) {
          hipLaunchKernelGGL(k_wide_children, dim3(blocks_of(u64(R) + 1, QUERY_THREADS)), T, 0, s, cur, F, start, R, W.head, W.depth, W.rank, W.ctrl);
          scan(W.rank, R + 1u);
          hipLaunchKernelGGL(k_wide_counts, dim3(blocks_of(u64(F) + 1, QUERY_THREADS)), T, 0, s, tape, cur, F, start, W.rank, W.count, W.ctrl);
          scan(W.count, F + 1u);
          WIDE_TRY(read_back(W.count + F, &next));
          if (next) {
            hipLaunchKernelGGL(k_wide_scatter, dim3(blocks_of(R, QUERY_THREADS)), T, 0, s, tape, cur, F, start, R, W.rank, reinterpret_cast<const u32 *>(W.count), out);
          }
        }
      } else {
        if (status_row) { hipLaunchKernelGGL(k_wide_status, dim3(blocks_of(F, QUERY_THREADS)), T, 0, s, table, docs, cur, F, u32(QUERY_INVALID_JSON_POINTER), status_row); }
        return hipSuccess; // ERR22 below the root: swallowed, nothing matches
      }
      if (lv.kind == PATH_TAIL || lv.kind == PATH_WILD_LAST) {
        *list = out;
        *count = next;
        return hipSuccess;
      }
      cur = out;
      F = next;
      flip ^= 1u;
    }
    return hipSuccess; // the frontier ran empty (or a program without a last level, which compile_path_program never leaves)
  };

  // first run: statuses, offsets, the total
  std::vector<u64> first_match(K);
  std::vector<u32> found(K);
  const u32 *list = W.roots;
  u64 running = 0;
  for (u32 k = 0; k < K; k++) {
    WIDE_TRY(hipMemsetAsync(status + size_t(k) * docs, 0, docs, s));
    u32 count = 0;
    WIDE_TRY(run_levels(k, true, &list, &count));
    first_match[k] = running;
    found[k] = count;
    hipLaunchKernelGGL(k_wide_offsets, dim3(blocks_of(u64(docs) + 1, QUERY_THREADS)), T, 0, s, table, docs, list, count, u32(running), k + 1u == K ? 1u : 0u,
                       offsets + size_t(k) * docs);
    running += count;
  }
  *matches_out = running;
  if (running <= 0xFFFFFFFFull && running <= match_cap) {
    // second run, writing.  The last path's list still lies where the first run left it: it goes first, before the blocks are used again
    for (u32 i = 0; i < K; i++) {
      const u32 k = i == 0 ? K - 1u : i - 1u;
      if (!found[k]) { continue; }
      u32 count = found[k];
      if (i) {
        WIDE_TRY(run_levels(k, false, &list, &count));
        count = count < found[k] ? count : found[k];
      }
      if (count) {
        hipLaunchKernelGGL(k_wide_emit, dim3(blocks_of(count, QUERY_THREADS)), T, 0, s, tape, string_buf, table, docs, list, count, value + first_match[k], tag + first_match[k]);
      }
    }
  }
  WIDE_TRY(hipGetLastError());
  return hipStreamSynchronize(s);
}
#undef WIDE_TRY

} // namespace sjgpu
