// simdjson_amd/csrc/sjgpu_json_wide.hip -- the JSON text of every cell of one row, breadth first (sjgpu_serialize_cells_wide_device): the outputs of
// sjgpu_serialize_cells_device (sjgpu_json.hip), bit for bit, with ONE LANE PER TAPE WORD where that call has one lane per cell.  Contract: include/sjgpu_json_wide.h.
//
// The words of the located container roots are laid end to end, every other root (a scalar, a code, a cell that disagrees with the tape) gets one slot: the RANGE
// SPACE, R slots.  Everything below the extents runs over it, one lane per slot, a workgroup of 256 lanes over 256 consecutive slots (a lane's share is 1 word, a
// wave's 64, a workgroup's 256).  A lane finds its root by a search in the scanned extents.
//   k_rows_locate      (sjgpu_query.hip, shared) what every root is
//   k_jw_extents       one lane per root: high - low words for a located container whose high index lies inside its document, else 1 (such a cell becomes a code 20)
//   k_gather_total, enqueue_scan   (shared) R in 64 bits -- read back: SJGPU_E_RANGE beyond 0xFFFFFFF0 -- and the roots' first slots
//   k_jw_marks, k_jw_carry_max, k_jw_heads   HEADS: a word is a number's second word exactly when the nearest word in front of it whose top byte is none of l u d
//                      lies at an even distance (the running-maximum rule of k_wide_ann_* in sjgpu_query.hip).  A root's first slot is a head by definition, so no run
//                      crosses a root.  Two levels: the workgroups' maxima, their exclusive running maximum by one workgroup, then every lane's own.
//   enqueue_scan       DEPTH: the exclusive sum of +1 for { [ and -1 for } ] over the heads; only the difference to the root's first slot is looked at
//   k_jw_maps, k_jw_carry_map, k_jw_count    KEYS AND COMMAS.  K[d]: "the container whose children lie at depth d is an object", P[d]: the parity of the heads seen at
//                      depth d, two 64-bit vectors.  A head at depth d toggles P[d]; an opening word also clears P[d + 1] and sets K[d + 1].  Every word is a map
//                      K' = (K & ~ck) | sk, P' = (P & ~cp) ^ tp, and two maps compose into one of the same form, so the state in front of every word is an exclusive scan
//                      of four u64, carried like the maximum.  From it: a string is a key when K[d] and P[d] is even; a : precedes the value behind a key, a , every
//                      other head that does not follow an opening word; a closing word reads the kind and the parity of the level it closes.
//                      k_jw_count then makes every check of walk_cell<false> as a predicate on its own word -- the ten tags, the string record inside its document's
//                      part of the buffer, a number's second word, a finite double, a key that is a string, the kind and the back pointer of a closing word, depth 0
//                      reached at the last word and never before -- OR-ed into a flag per root, and the length of its word's text: prefix byte and text.
//                      The parallel state equals the walk's up to the first violation, so "some word violates" and "the walk returns false" are one verdict.
//   k_jw_roots         one lane per root: status 20 for a flagged root.  A root that nests 64 or more levels below itself is handed, whole, to the one-lane walk
//                      (sj_json_walk.h, shared with sjgpu_json.hip): its length lands on its first slot, its other slots count 0
//   k_jw_settle        one lane per slot: the slots of a flagged root count 0; the 64-bit sums
//   k_gather_total, enqueue_scan   (shared) the slots' offsets in place and the total in 64 bits
//   k_jw_offsets       offsets[r] = the offset of root r's first slot
//   k_jw_fill          one lane per head, writing at its own offset and never at or beyond the next one's; k_jw_fill_deep: the one-lane walk for the deep roots
// The number of launches depends neither on the data nor on the nesting depth; every loop is bounded by log2(rows), by a string's length or by a number's 20 digits,
// except the walk of a root deeper than 63 levels; nobody waits for anybody.  A string is still one lane's work, and so is a double, converted in both passes.
// PRETTY = true: sjgpu_prettify_cells_wide_device (include/sjgpu_pretty.h).  The layout of a word is a function of what k_jw_count knows already -- the
// depth d, the kind and the parity of its level -- and of one fact more, whether the word in front of a closing word opened it: pre[r] then holds a code, not a byte
// (jw_layout below), and k_jw_fill writes the newline, the indent, the blank behind a key's colon and the closing newline from it.  No launch more, no byte of workspace more.
// The staged road of k_write_fill (a workgroup's span through LDS, 16-byte stores) is NOT built: k_jw_fill writes direct stores.
#include "sjgpu_device.h"
#include "sjgpu_json_wide.h"
#include "sj_json_text.h"
#include "sj_query_program.h"
#include "sj_json_walk.h"

namespace sjgpu {
namespace {

constexpr u32 JW_THREADS = 256, JW_WAVES = JW_THREADS / 64;
constexpr u32 JW_BAD = 1u, JW_DEEP = 2u; // a root's flags
constexpr u32 JW_LEVELS = 64;            // the levels below a root that the two vectors hold

// PRETTY, what stands around a word's text, in pre[r]: bits 0-2 what lies in front, bits 3-6 the level l whose 4 l blanks follow a newline, bit 7 a newline behind
constexpr u32 JW_NONE = 0, JW_COMMA = 1, JW_COLON = 2, JW_COLON_BLANK = 3, JW_LINE = 4, JW_COMMA_LINE = 5;
__device__ __forceinline__ u32 jw_layout(u32 front, u32 l, bool line_behind) { return front | (l << 3) | (line_behind ? 128u : 0u); }
__device__ __forceinline__ u32 jw_layout_bytes(u32 p) {
  const u32 front = p & 7u, indent = 4u * ((p >> 3) & 15u);
  return (front == JW_NONE ? 0u : front == JW_COMMA || front == JW_COLON ? 1u : front == JW_COLON_BLANK ? 2u : front == JW_LINE ? 1u + indent : 2u + indent) + (p >> 7);
}
__device__ __forceinline__ bool jw_is_number(u32 t) { return t == 'l' || t == 'u' || t == 'd'; }
__device__ __forceinline__ bool jw_opens(u32 t) { return t == '{' || t == '['; }
__device__ __forceinline__ bool jw_closes(u32 t) { return t == '}' || t == ']'; }
__device__ __forceinline__ u32 jw_max(u32 a, u32 b) { return a > b ? a : b; }
static inline u32 jw_blocks(u64 n) { return u32((n + JW_THREADS - 1) / JW_THREADS); }

// the root of slot r: the LAST e with start[e] <= r (start[0] = 0, every root has a slot, so the starts ascend strictly)
__device__ __forceinline__ u32 jw_owner(const u32 *__restrict__ start, u32 rows, u32 r) {
  u32 lo = 0, hi = rows;
  while (hi - lo > 1u) {
    const u32 mid = lo + (hi - lo) / 2u;
    if (start[mid] <= r) { lo = mid; } else { hi = mid; }
  }
  return lo;
}

// slot r as every kernel sees it: its root e, its place j among the root's ext slots, and -- for a located container -- its tape word w at index i
struct jw_slot {
  u32 e, j, ext, m;
  u64 low, i, w;
  bool container;
};
__device__ __forceinline__ jw_slot jw_slot_of(const u64 *__restrict__ tape, const u64 *__restrict__ root_value, const u32 *__restrict__ where, const u32 *__restrict__ start,
                                              u32 rows, u32 r) {
  jw_slot s;
  s.e = jw_owner(start, rows, r);
  s.j = r - start[s.e];
  s.ext = start[s.e + 1u] - start[s.e];
  s.m = where[s.e];
  s.container = s.m < ROWS_SPECIAL;
  s.low = 0;
  s.i = 0;
  s.w = 0;
  if (s.container) {
    s.low = root_value[s.e] & LOW32;
    s.i = s.low + s.j; // (below the cell's high index, which k_jw_extents found inside the document)
    s.w = tape[s.i];
  }
  return s;
}
// r + 1 for a slot behind which a head must come: a root's first slot, a slot of its own, a word whose top byte is none of l u d
__device__ __forceinline__ u32 jw_mark(const jw_slot &s, u32 r) { return !s.container || s.j == 0 || !jw_is_number(u32(s.w >> 56)) ? r + 1u : 0u; }

// ---- the extents -------------------------------------------------------------------------------------------------------------------------------------------------
// ext[e] for e < rows, ext[rows] = 0; block_sums[workgroup] = its extents in 64 bits.  A located container whose high index is not behind its low one or lies beyond
// its document becomes the code 20 that the walk would have given it
__global__ __launch_bounds__(JW_THREADS) void k_jw_extents(const doc_span_dev *__restrict__ table, const u64 *__restrict__ root_value, u32 *__restrict__ where, u32 rows,
                                                           u32 *__restrict__ ext, u64 *__restrict__ block_sums) {
  __shared__ u64 s_sum[JW_WAVES];
  const u64 e = u64(blockIdx.x) * JW_THREADS + threadIdx.x;
  u64 words = 0;
  if (e < rows) {
    words = 1;
    const u32 m = where[e];
    if (m < ROWS_SPECIAL) {
      const u64 v = root_value[e], low = v & LOW32, high = v >> 32;
      if (high > low && high <= table[m + 1u].tape_begin) {
        words = high - low;
      } else {
        where[e] = ROWS_SPECIAL | (QUERY_NO_SUCH_FIELD - 16u);
      }
    }
  }
  if (e <= rows) { ext[e] = u32(words); }
  u64 sum = words;
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) { sum += __shfl_xor(sum, x); }
  if (lane_id() == 0) { s_sum[threadIdx.x >> 6] = sum; }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) { block_sums[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]; }
}

// ---- the heads ---------------------------------------------------------------------------------------------------------------------------------------------------
// share_last[b] = the largest mark of workgroup b's slots
__global__ __launch_bounds__(JW_THREADS) void k_jw_marks(const u64 *__restrict__ tape, const u64 *__restrict__ root_value, const u32 *__restrict__ where,
                                                         const u32 *__restrict__ start, u32 rows, u32 R, u32 *__restrict__ share_last) {
  __shared__ u32 s_max[JW_WAVES];
  const u64 r = u64(blockIdx.x) * JW_THREADS + threadIdx.x;
  u32 m = 0;
  if (r < R) { m = jw_mark(jw_slot_of(tape, root_value, where, start, rows, u32(r)), u32(r)); }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) { m = jw_max(m, __shfl_xor(m, x)); }
  if (lane_id() == 0) { s_max[threadIdx.x >> 6] = m; }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) { share_last[blockIdx.x] = jw_max(jw_max(s_max[0], s_max[1]), jw_max(s_max[2], s_max[3])); }
}
// one workgroup, in place: share_last[b] becomes the largest mark IN FRONT of workgroup b's slots
__global__ __launch_bounds__(JW_THREADS) void k_jw_carry_max(u32 *__restrict__ share_last, u32 shares) {
  __shared__ u32 s_part[JW_THREADS];
  const u32 per = (shares + JW_THREADS - 1u) / JW_THREADS;
  const u32 lo = min(threadIdx.x * per, shares), hi = min(lo + per, shares);
  u32 m = 0;
  for (u32 i = lo; i < hi; i++) { m = jw_max(m, share_last[i]); }
  s_part[threadIdx.x] = m;
  lds_writes_done();
  __syncthreads();
  u32 run = 0;
  for (u32 t = 0; t < threadIdx.x; t++) { run = jw_max(run, s_part[t]); }
  for (u32 i = lo; i < hi; i++) {
    const u32 x = share_last[i];
    share_last[i] = run;
    run = jw_max(run, x);
  }
}
// head[r] and, in depth[r], the slot's +1 / -1 / 0 (the scan behind this kernel makes it the depth); *scan_n = R
__global__ __launch_bounds__(JW_THREADS) void k_jw_heads(const u64 *__restrict__ tape, const u64 *__restrict__ root_value, const u32 *__restrict__ where,
                                                         const u32 *__restrict__ start, u32 rows, u32 R, const u32 *__restrict__ share_carry, u8 *__restrict__ head,
                                                         int *__restrict__ depth, u32 *__restrict__ scan_n) {
  __shared__ u32 s_wave[JW_WAVES];
  const u64 r64 = u64(blockIdx.x) * JW_THREADS + threadIdx.x;
  const bool live = r64 < R;
  const u32 r = u32(r64);
  jw_slot s = {};
  u32 mark = 0;
  if (live) {
    s = jw_slot_of(tape, root_value, where, start, rows, r);
    mark = jw_mark(s, r);
  }
  u32 incl = mark; // the running maximum over the lanes of the wave
#pragma unroll
  for (u32 d = 1; d < 64; d <<= 1) {
    const u32 other = __shfl_up(incl, d);
    if (lane_id() >= d) { incl = jw_max(incl, other); }
  }
  u32 run = __shfl_up(incl, 1u);
  if (lane_id() == 0) { run = 0; }
  if (lane_id() == 63) { s_wave[threadIdx.x >> 6] = incl; }
  lds_writes_done();
  __syncthreads();
  run = jw_max(run, share_carry[blockIdx.x]);
  for (u32 v = 0; v < (threadIdx.x >> 6); v++) { run = jw_max(run, s_wave[v]); }
  if (live) {
    const bool is_head = !s.container || s.j == 0 || ((r - run) & 1u) == 0;
    const u32 t = u32(s.w >> 56);
    head[r] = is_head ? 1 : 0;
    depth[r] = !is_head || !s.container ? 0 : (jw_opens(t) ? 1 : (jw_closes(t) ? -1 : 0));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { *scan_n = R; }
}

// ---- keys and commas ---------------------------------------------------------------------------------------------------------------------------------------------
struct jw_map {
  u64 ck, sk, cp, tp;
};
// a, then b
__device__ __forceinline__ jw_map jw_then(const jw_map &a, const jw_map &b) {
  jw_map c;
  c.ck = a.ck | b.ck;
  c.sk = (a.sk & ~b.ck) | b.sk;
  c.cp = a.cp | b.cp;
  c.tp = (a.tp & ~b.cp) ^ b.tp;
  return c;
}
// the map of one word: a head tagged t at depth d below its root's first slot
__device__ __forceinline__ jw_map jw_word_map(bool is_head, u32 t, u32 d) {
  jw_map m = {0, 0, 0, 0};
  if (!is_head || d >= JW_LEVELS || jw_closes(t)) { return m; }
  m.tp = 1ull << d;
  if (jw_opens(t) && d + 1u < JW_LEVELS) {
    const u64 below = 2ull << d;
    m.ck = below;
    m.cp = below;
    m.sk = t == '{' ? below : 0;
  }
  return m;
}
// the maps of the wave's lanes up to and including this one
__device__ __forceinline__ jw_map jw_wave_inclusive(jw_map incl) {
#pragma unroll
  for (u32 d = 1; d < 64; d <<= 1) {
    jw_map front;
    front.ck = __shfl_up(incl.ck, d);
    front.sk = __shfl_up(incl.sk, d);
    front.cp = __shfl_up(incl.cp, d);
    front.tp = __shfl_up(incl.tp, d);
    if (lane_id() >= d) { incl = jw_then(front, incl); }
  }
  return incl;
}
// slot r's own map and what it is; a word 64 or more levels below its root flags the root DEEP (flag: null in the kernels behind the first)
__device__ __forceinline__ jw_map jw_slot_map(const jw_slot &s, u32 r, const u32 *__restrict__ start, const u8 *__restrict__ head, const int *__restrict__ depth,
                                              u32 *__restrict__ root_flag, u32 *d_out, bool *head_out) {
  const jw_map none = {0, 0, 0, 0};
  *d_out = 0;
  *head_out = true;
  if (!s.container) { return none; }
  const u32 d = u32(depth[r]) - u32(depth[start[s.e]]);
  *d_out = d;
  *head_out = head[r] != 0;
  if (d >= JW_LEVELS) {
    if (root_flag) { atomicOr(&root_flag[s.e], JW_DEEP); }
    return none;
  }
  return jw_word_map(*head_out, u32(s.w >> 56), d);
}

// share_map[b] = the maps of workgroup b's slots, composed in order; the DEEP flags
__global__ __launch_bounds__(JW_THREADS) void k_jw_maps(const u64 *__restrict__ tape, const u64 *__restrict__ root_value, const u32 *__restrict__ where,
                                                        const u32 *__restrict__ start, u32 rows, u32 R, const u8 *__restrict__ head, const int *__restrict__ depth,
                                                        u32 *__restrict__ root_flag, jw_map *__restrict__ share_map) {
  __shared__ jw_map s_wave[JW_WAVES];
  const u64 r64 = u64(blockIdx.x) * JW_THREADS + threadIdx.x;
  jw_map own = {0, 0, 0, 0};
  if (r64 < R) {
    const u32 r = u32(r64);
    const jw_slot s = jw_slot_of(tape, root_value, where, start, rows, r);
    u32 d;
    bool is_head;
    own = jw_slot_map(s, r, start, head, depth, root_flag, &d, &is_head);
  }
  const jw_map incl = jw_wave_inclusive(own);
  if (lane_id() == 63) { s_wave[threadIdx.x >> 6] = incl; }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) { share_map[blockIdx.x] = jw_then(jw_then(s_wave[0], s_wave[1]), jw_then(s_wave[2], s_wave[3])); }
}
// one workgroup, in place: share_map[b] becomes the composition of the maps IN FRONT of workgroup b
__global__ __launch_bounds__(JW_THREADS) void k_jw_carry_map(jw_map *__restrict__ share_map, u32 shares) {
  __shared__ jw_map s_part[JW_THREADS];
  const u32 per = (shares + JW_THREADS - 1u) / JW_THREADS;
  const u32 lo = min(threadIdx.x * per, shares), hi = min(lo + per, shares);
  jw_map m = {0, 0, 0, 0};
  for (u32 i = lo; i < hi; i++) { m = jw_then(m, share_map[i]); }
  s_part[threadIdx.x] = m;
  lds_writes_done();
  __syncthreads();
  jw_map run = {0, 0, 0, 0};
  for (u32 t = 0; t < threadIdx.x; t++) { run = jw_then(run, s_part[t]); }
  for (u32 i = lo; i < hi; i++) {
    const jw_map x = share_map[i];
    share_map[i] = run;
    run = jw_then(run, x);
  }
}

// the string record of word w inside [str_base, str_end) -> true with where its bytes begin and how many they are
__device__ __forceinline__ bool jw_string_record(const u8 *__restrict__ sbuf, u64 w, u64 str_base, u64 str_end, u64 *at, u32 *len) {
  const u64 rec = str_base + (w & PAYLOAD);
  if (rec + 4u > str_end) { return false; }
  *len = *reinterpret_cast<const u32_unaligned *>(sbuf + rec);
  *at = rec + 4u;
  return rec + 4u + u64(*len) <= str_end;
}

// len[r] = the low 32 bits of the length of slot r's text, pre[r] = the byte in front of it (0 , :); what is above 32 bits is added to root_high[e]; a word that the
// walk would refuse flags its root BAD.  A slot of its own is served here as serialize_root serves it, with its status
// PRETTY: pre[r] = jw_layout of what stands around the word's text, and the length counts it
template <bool PRETTY>
__global__ __launch_bounds__(JW_THREADS) void k_jw_count(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 string_bytes, const doc_span_dev *__restrict__ table,
                                                         const u64 *__restrict__ root_value, const u8 *__restrict__ root_tag, const u32 *__restrict__ where,
                                                         const u32 *__restrict__ start, u32 rows, u32 R, const u8 *__restrict__ head, const int *__restrict__ depth,
                                                         const jw_map *__restrict__ share_carry, u32 *__restrict__ root_flag, u32 *__restrict__ root_high,
                                                         u32 *__restrict__ len, u8 *__restrict__ pre, u8 *__restrict__ status) {
  __shared__ jw_map s_wave[JW_WAVES];
  const u64 r64 = u64(blockIdx.x) * JW_THREADS + threadIdx.x;
  const bool live = r64 < R;
  const u32 r = u32(r64);
  jw_slot s = {};
  jw_map own = {0, 0, 0, 0};
  u32 d = 0;
  bool is_head = false;
  if (live) {
    s = jw_slot_of(tape, root_value, where, start, rows, r);
    own = jw_slot_map(s, r, start, head, depth, nullptr, &d, &is_head);
  }
  const jw_map incl = jw_wave_inclusive(own);
  jw_map front;
  front.ck = __shfl_up(incl.ck, 1u);
  front.sk = __shfl_up(incl.sk, 1u);
  front.cp = __shfl_up(incl.cp, 1u);
  front.tp = __shfl_up(incl.tp, 1u);
  if (lane_id() == 0) { front = jw_map{0, 0, 0, 0}; }
  if (lane_id() == 63) { s_wave[threadIdx.x >> 6] = incl; }
  lds_writes_done();
  __syncthreads();
  jw_map before = share_carry[blockIdx.x];
  for (u32 v = 0; v < (threadIdx.x >> 6); v++) { before = jw_then(before, s_wave[v]); }
  before = jw_then(before, front);
  if (!live) { return; }
  const u64 K = before.sk, P = before.tp; // the state in front of this word: the maps applied to nothing
  u64 length = 0;
  u32 prefix = 0;
  bool bad = false;
  if (!s.container) {
    json_sink<false> sink = {nullptr, 0, 0};
    status[s.e] = u8(serialize_root<false, PRETTY>(tape, sbuf, string_bytes, table, s.m, root_tag[s.e], root_value[s.e], nullptr, sink));
    length = sink.at;
  } else if (!(root_flag[s.e] & JW_DEEP) && is_head) {
    const u32 t = u32(s.w >> 56);
    const uint4 a = *reinterpret_cast<const uint4 *>(table + s.m), b = *reinterpret_cast<const uint4 *>(table + s.m + 1u);
    const u64 base = a.z, str_base = a.w, str_end = b.w;
    const bool in_object = (K >> d) & 1u, odd = (P >> d) & 1u, last = s.j + 1u == s.ext;
    if (jw_closes(t)) {
      bad = d == 0 || in_object != (t == '}') || (in_object && odd) || (d == 1u) != last;
      const u64 o = base + (s.w & LOW32);
      if (o < s.low || o >= s.i) {
        bad = true;
      } else {
        const u64 ow = tape[o];
        bad = bad || u32(ow >> 56) != (in_object ? u32('{') : u32('[')) || base + (ow & LOW32) != s.i + 1u;
      }
      length = 1;
      if (PRETTY && d != 0) {
        const u32 l = (d - 1u) & 15u; // the level of the container that closes here
        const bool empty = head[r - 1u] != 0 && jw_opens(u32(tape[s.i - 1u] >> 56)); // (d != 0: a word of this root lies in front)
        const u32 front = !empty && l != 15u ? JW_LINE : JW_NONE;
        prefix = jw_layout(front, l, l == 0);
        length += jw_layout_bytes(prefix);
      }
    } else {
      bad = last || (s.j != 0 && d == 0); // the last word closes the root, and nothing else stands at its level
      if (s.j != 0) {
        const bool is_key = in_object && !odd;
        bad = bad || (is_key && t != '"');
        const bool first = head[r - 1u] != 0 && jw_opens(u32(tape[s.i - 1u] >> 56));
        prefix = first ? 0u : (in_object && odd ? u32(':') : u32(','));
        if (PRETTY) {
          const u32 l = d & 15u;
          const bool flat = l == 0; // (d != 0 behind a root's first slot, or the root is BAD: the parent is a container with l = 15)
          const u32 front = in_object && odd ? (flat ? JW_COLON : JW_COLON_BLANK) : first ? (flat ? JW_NONE : JW_LINE) : (flat ? JW_COMMA : JW_COMMA_LINE);
          prefix = jw_layout(front, l, flat && !is_key && !jw_opens(t));
        }
      }
      if (jw_opens(t)) {
        length = 1;
      } else if (t == '"') {
        u64 at;
        u32 n;
        if (jw_string_record(sbuf, s.w, str_base, str_end, &at, &n)) { length = escaped_length(sbuf + at, n); } else { bad = true; }
      } else if (jw_is_number(t)) {
        if (last) {
          bad = true; // (no second word)
        } else {
          const u64 v = tape[s.i + 1u];
          if (t == 'd' && !dtoa_is_finite(v)) { bad = true; } else { length = t == 'd' ? dtoa_length(v) : t == 'l' ? int64_text_length(v) : decimal_digits(v); }
        }
      } else if (t == 't' || t == 'n') {
        length = 4;
      } else if (t == 'f') {
        length = 5;
      } else {
        bad = true;
      }
      length += PRETTY ? jw_layout_bytes(prefix) : (prefix ? 1u : 0u);
    }
  } else if (!(root_flag[s.e] & JW_DEEP)) {
    bad = s.j + 1u == s.ext; // a number's second word where the closing word belongs
  }
  len[r] = u32(length);
  pre[r] = u8(prefix);
  if (length >> 32) { atomicAdd(&root_high[s.e], u32(length >> 32)); }
  if (bad) { atomicOr(&root_flag[s.e], JW_BAD); }
}

// one lane per located container root, grid-stride: its status; a DEEP root is walked by this lane, its length on its first slot
template <bool PRETTY>
__global__ __launch_bounds__(JSON_THREADS) void k_jw_roots(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 string_bytes, const doc_span_dev *__restrict__ table,
                                                           const u64 *__restrict__ root_value, const u8 *__restrict__ root_tag, const u32 *__restrict__ where,
                                                           const u32 *__restrict__ start, u32 rows, const u32 *__restrict__ root_flag, u32 *__restrict__ root_high,
                                                           u64 *__restrict__ strips, u32 *__restrict__ len, u8 *__restrict__ status) {
  const u64 lane_global = u64(blockIdx.x) * JSON_THREADS + threadIdx.x, stride = u64(gridDim.x) * JSON_THREADS;
  u64 *strip = strips + lane_global * JSON_STRIP_WORDS;
  for (u64 e = lane_global; e < rows; e += stride) {
    const u32 m = where[e];
    if (m >= ROWS_SPECIAL) { continue; } // (k_jw_count served it)
    const u32 f = root_flag[e];
    u32 code = f & JW_BAD ? QUERY_NO_SUCH_FIELD : 0u;
    if (f & JW_DEEP) {
      json_sink<false> sink = {nullptr, 0, 0};
      code = serialize_root<false, PRETTY>(tape, sbuf, string_bytes, table, m, root_tag[e], root_value[e], strip, sink);
      len[start[e]] = u32(sink.at);
      root_high[e] = u32(sink.at >> 32);
    }
    status[e] = u8(code);
  }
}

// one lane per slot: the slots of a BAD root that was not walked count 0; len[R] = 0; block_sums[workgroup] = its lengths in 64 bits
__global__ __launch_bounds__(JW_THREADS) void k_jw_settle(const u32 *__restrict__ where, const u32 *__restrict__ start, u32 rows, u32 R, const u32 *__restrict__ root_flag,
                                                          const u32 *__restrict__ root_high, u32 *__restrict__ len, u64 *__restrict__ block_sums) {
  __shared__ u64 s_sum[JW_WAVES];
  const u64 r64 = u64(blockIdx.x) * JW_THREADS + threadIdx.x;
  u64 sum = 0;
  if (r64 < R) {
    const u32 r = u32(r64), e = jw_owner(start, rows, r);
    if (where[e] < ROWS_SPECIAL && (root_flag[e] & (JW_BAD | JW_DEEP)) == JW_BAD) {
      len[r] = 0;
    } else {
      sum = len[r];
      if (r == start[e]) { sum += u64(root_high[e]) << 32; }
    }
  } else if (r64 == R) {
    len[R] = 0;
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) { sum += __shfl_xor(sum, x); }
  if (lane_id() == 0) { s_sum[threadIdx.x >> 6] = sum; }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) { block_sums[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]; }
}

// offsets[e] = where root e's text begins, offsets[rows] = the total's low 32 bits (off: the scanned lengths, R + 1 of them)
__global__ __launch_bounds__(JW_THREADS) void k_jw_offsets(const u32 *__restrict__ start, u32 rows, const u32 *__restrict__ off, u32 *__restrict__ offsets) {
  const u64 e = u64(blockIdx.x) * JW_THREADS + threadIdx.x;
  if (e <= rows) { offsets[e] = off[start[e]]; }
}

// one lane per slot with bytes: chars[off[r] .. off[r + 1])
template <bool PRETTY>
__global__ __launch_bounds__(JW_THREADS) void k_jw_fill(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 string_bytes, const doc_span_dev *__restrict__ table,
                                                        const u64 *__restrict__ root_value, const u8 *__restrict__ root_tag, const u32 *__restrict__ where,
                                                        const u32 *__restrict__ start, u32 rows, u32 R, const u32 *__restrict__ root_flag, const u32 *__restrict__ off,
                                                        const u8 *__restrict__ pre, u8 *__restrict__ chars) {
  const u64 r64 = u64(blockIdx.x) * JW_THREADS + threadIdx.x;
  if (r64 >= R) { return; }
  const u32 r = u32(r64);
  const u64 begin = off[r], end = off[r + 1u];
  if (begin >= end) { return; }
  const jw_slot s = jw_slot_of(tape, root_value, where, start, rows, r);
  json_sink<true> sink = {chars + begin, end - begin, 0};
  if (!s.container) {
    (void)serialize_root<true, PRETTY>(tape, sbuf, string_bytes, table, s.m, root_tag[s.e], root_value[s.e], nullptr, sink);
    return;
  }
  if (root_flag[s.e] & JW_DEEP) { return; } // (k_jw_fill_deep writes it)
  const u32 t = u32(s.w >> 56), prefix = pre[r];
  if (PRETTY) {
    const u32 front = prefix & 7u;
    if (front == JW_COMMA || front == JW_COMMA_LINE) { sink.put(','); }
    if (front == JW_COLON || front == JW_COLON_BLANK) { sink.put(':'); }
    if (front == JW_COLON_BLANK) { sink.put(' '); }
    if (front == JW_LINE || front == JW_COMMA_LINE) {
      sink.put('\n');
      sink.put_spaces(4u * ((prefix >> 3) & 15u));
    }
  } else if (prefix) {
    sink.put(prefix);
  }
  if (jw_opens(t) || jw_closes(t)) {
    sink.put(t);
  } else if (t == '"') {
    const uint4 a = *reinterpret_cast<const uint4 *>(table + s.m), b = *reinterpret_cast<const uint4 *>(table + s.m + 1u);
    u64 at;
    u32 n;
    if (jw_string_record(sbuf, s.w, a.w, b.w, &at, &n)) { sink.put_string(sbuf + at, n); }
  } else if (jw_is_number(t)) {
    if (s.j + 1u < s.ext) { sink.put_number(t, tape[s.i + 1u]); }
  } else {
    sink.put_literal(t);
  }
  if (PRETTY && (prefix >> 7)) { sink.put('\n'); }
}
// the grid of k_jw_roots: the bytes of a DEEP root, by the walk that counted them
template <bool PRETTY>
__global__ __launch_bounds__(JSON_THREADS) void k_jw_fill_deep(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 string_bytes, const doc_span_dev *__restrict__ table,
                                                               const u64 *__restrict__ root_value, const u8 *__restrict__ root_tag, const u32 *__restrict__ where,
                                                               const u32 *__restrict__ start, u32 rows, const u32 *__restrict__ root_flag, u64 *__restrict__ strips,
                                                               const u32 *__restrict__ off, u8 *__restrict__ chars) {
  const u64 lane_global = u64(blockIdx.x) * JSON_THREADS + threadIdx.x, stride = u64(gridDim.x) * JSON_THREADS;
  u64 *strip = strips + lane_global * JSON_STRIP_WORDS;
  for (u64 e = lane_global; e < rows; e += stride) {
    const u32 m = where[e];
    if (m >= ROWS_SPECIAL || !(root_flag[e] & JW_DEEP)) { continue; }
    const u64 begin = off[start[e]], end = off[start[e] + 1u]; // (its other slots have no bytes)
    if (begin >= end) { continue; }
    json_sink<true> sink = {chars + begin, end - begin, 0};
    (void)serialize_root<true, PRETTY>(tape, sbuf, string_bytes, table, m, root_tag[e], root_value[e], strip, sink);
  }
}

static inline u32 walk_blocks(u32 rows) {
  const u64 all = (u64(rows) + JSON_THREADS - 1) / JSON_THREADS;
  return u32(all < JSON_MAX_WORKGROUPS ? all : JSON_MAX_WORKGROUPS);
}
static inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// per root: [ctrl, 256 bytes][where][start: rows + 1][flags][high words][the extents' block sums][the scan's block sums]
struct jw_root_space {
  count_total_dev *ctrl;
  u32 *where, *start, *flag, *high;
  u64 *block_sums;
  int *partial;
  size_t bytes;
};
static inline jw_root_space carve_roots(void *base, u32 rows) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(base);
  size_t at = 0;
  auto take = [&](size_t n) {
    void *q = reinterpret_cast<void *>(p + at);
    at += up256(n);
    return q;
  };
  jw_root_space w;
  w.ctrl = static_cast<count_total_dev *>(take(256));
  w.where = static_cast<u32 *>(take(size_t(rows) * 4));
  w.start = static_cast<u32 *>(take((size_t(rows) + 1) * 4));
  w.flag = static_cast<u32 *>(take(size_t(rows) * 4));
  w.high = static_cast<u32 *>(take(size_t(rows) * 4));
  w.block_sums = static_cast<u64 *>(take(size_t(jw_blocks(u64(rows) + 1)) * 8));
  w.partial = static_cast<int *>(take((size_t((u64(rows) + 1 + 4095) / 4096) + 64) * 4));
  w.bytes = at;
  return w;
}
// per slot: [ctrl, 256 bytes][head: 1][depth: 4][len: 4, R + 1 of them][pre: 1][per workgroup: its mark 4, its map 32, its sum 8][the scans' block sums]
// [the strips of the lanes that walk deep roots]
struct jw_word_space {
  count_total_dev *ctrl;
  u32 *scan_n;
  u8 *head, *pre;
  int *depth;
  u32 *len, *share_max;
  jw_map *share_map;
  u64 *block_sums, *strips;
  int *partial;
  size_t bytes;
};
static inline jw_word_space carve_words(void *base, u32 rows, u64 R) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(base);
  size_t at = 0;
  auto take = [&](size_t n) {
    void *q = reinterpret_cast<void *>(p + at);
    at += up256(n);
    return q;
  };
  const size_t shares = jw_blocks(R + 1);
  jw_word_space w;
  w.ctrl = static_cast<count_total_dev *>(take(256));
  w.scan_n = reinterpret_cast<u32 *>(w.ctrl + 1);
  w.head = static_cast<u8 *>(take(size_t(R)));
  w.depth = static_cast<int *>(take(size_t(R) * 4));
  w.len = static_cast<u32 *>(take((size_t(R) + 1) * 4));
  w.pre = static_cast<u8 *>(take(size_t(R)));
  w.share_max = static_cast<u32 *>(take(shares * 4));
  w.share_map = static_cast<jw_map *>(take(shares * sizeof(jw_map)));
  w.block_sums = static_cast<u64 *>(take(shares * 8));
  w.partial = static_cast<int *>(take((size_t((R + 1 + 4095) / 4096) + 64) * 4));
  w.strips = static_cast<u64 *>(take(size_t(walk_blocks(rows)) * JSON_THREADS * JSON_STRIP_WORDS * sizeof(u64)));
  w.bytes = at;
  return w;
}

} // namespace

size_t json_wide_root_bytes(uint32_t rows) { return carve_roots(nullptr, rows).bytes; }
size_t json_wide_word_bytes(uint32_t rows, uint64_t range_words) { return carve_words(nullptr, rows, range_words).bytes; }
uint32_t *json_wide_where(void *root_space, uint32_t rows) { return carve_roots(root_space, rows).where; }
uint32_t json_wide_share() { return JW_THREADS; }

const count_total_dev *launch_json_wide_extents(const uint64_t *tape, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag, uint32_t rows,
                                                void *root_space, hipStream_t s) {
  const jw_root_space w = carve_roots(root_space, rows);
  const u32 blocks = jw_blocks(u64(rows) + 1);
  launch_rows_locate(tape, table, docs, root_value, root_tag, rows, w.where, s);
  hipLaunchKernelGGL(k_jw_extents, dim3(blocks), dim3(JW_THREADS), 0, s, table, root_value, w.where, rows, w.start, w.block_sums);
  launch_count_total(w.block_sums, blocks, rows, w.ctrl, s);
  enqueue_scan(reinterpret_cast<int *>(w.start), rows + 1u, &w.ctrl->n_plus_1, w.partial, s);
  return w.ctrl;
}

namespace {
template <bool PRETTY>
hipError_t json_wide_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value,
                           const uint8_t *root_tag, uint32_t rows, uint64_t range_words, uint32_t *offsets, uint8_t *status, void *root_space, void *word_space,
                           hipStream_t s, const count_total_dev **total) {
  const jw_root_space A = carve_roots(root_space, rows);
  const jw_word_space W = carve_words(word_space, rows, range_words);
  const u32 R = u32(range_words), shares = jw_blocks(range_words), blocks1 = jw_blocks(range_words + 1);
  const dim3 T(JW_THREADS);
  *total = W.ctrl;
  hipError_t e = hipMemsetAsync(A.flag, 0, size_t(rows) * 4, s);
  if (e != hipSuccess) { return e; }
  e = hipMemsetAsync(A.high, 0, size_t(rows) * 4, s);
  if (e != hipSuccess) { return e; }
  hipLaunchKernelGGL(k_jw_marks, dim3(shares), T, 0, s, tape, root_value, static_cast<const u32 *>(A.where), static_cast<const u32 *>(A.start), rows, R, W.share_max);
  hipLaunchKernelGGL(k_jw_carry_max, dim3(1), T, 0, s, W.share_max, shares);
  hipLaunchKernelGGL(k_jw_heads, dim3(shares), T, 0, s, tape, root_value, static_cast<const u32 *>(A.where), static_cast<const u32 *>(A.start), rows, R,
                     static_cast<const u32 *>(W.share_max), W.head, W.depth, W.scan_n);
  enqueue_scan(W.depth, R, W.scan_n, W.partial, s);
  hipLaunchKernelGGL(k_jw_maps, dim3(shares), T, 0, s, tape, root_value, static_cast<const u32 *>(A.where), static_cast<const u32 *>(A.start), rows, R,
                     static_cast<const u8 *>(W.head), static_cast<const int *>(W.depth), A.flag, W.share_map);
  hipLaunchKernelGGL(k_jw_carry_map, dim3(1), T, 0, s, W.share_map, shares);
  hipLaunchKernelGGL(k_jw_count<PRETTY>, dim3(shares), T, 0, s, tape, string_buf, string_bytes, table, root_value, root_tag, static_cast<const u32 *>(A.where),
                     static_cast<const u32 *>(A.start), rows, R, static_cast<const u8 *>(W.head), static_cast<const int *>(W.depth), static_cast<const jw_map *>(W.share_map),
                     A.flag, A.high, W.len, W.pre, status);
  hipLaunchKernelGGL(k_jw_roots<PRETTY>, dim3(walk_blocks(rows)), dim3(JSON_THREADS), 0, s, tape, string_buf, string_bytes, table, root_value, root_tag,
                     static_cast<const u32 *>(A.where), static_cast<const u32 *>(A.start), rows, static_cast<const u32 *>(A.flag), A.high, W.strips, W.len, status);
  hipLaunchKernelGGL(k_jw_settle, dim3(blocks1), T, 0, s, static_cast<const u32 *>(A.where), static_cast<const u32 *>(A.start), rows, R, static_cast<const u32 *>(A.flag),
                     static_cast<const u32 *>(A.high), W.len, W.block_sums);
  launch_count_total(W.block_sums, blocks1, R, W.ctrl, s);
  enqueue_scan(reinterpret_cast<int *>(W.len), R + 1u, &W.ctrl->n_plus_1, W.partial, s);
  hipLaunchKernelGGL(k_jw_offsets, dim3(jw_blocks(u64(rows) + 1)), T, 0, s, static_cast<const u32 *>(A.start), rows, static_cast<const u32 *>(W.len), offsets);
  return hipSuccess;
}

template <bool PRETTY>
void json_wide_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                    uint32_t rows, uint64_t range_words, uint8_t *chars, void *root_space, void *word_space, hipStream_t s) {
  const jw_root_space A = carve_roots(root_space, rows);
  const jw_word_space W = carve_words(word_space, rows, range_words);
  const u32 R = u32(range_words);
  hipLaunchKernelGGL(k_jw_fill<PRETTY>, dim3(jw_blocks(range_words)), dim3(JW_THREADS), 0, s, tape, string_buf, string_bytes, table, root_value, root_tag,
                     static_cast<const u32 *>(A.where), static_cast<const u32 *>(A.start), rows, R, static_cast<const u32 *>(A.flag), static_cast<const u32 *>(W.len),
                     static_cast<const u8 *>(W.pre), chars);
  hipLaunchKernelGGL(k_jw_fill_deep<PRETTY>, dim3(walk_blocks(rows)), dim3(JSON_THREADS), 0, s, tape, string_buf, string_bytes, table, root_value, root_tag,
                     static_cast<const u32 *>(A.where), static_cast<const u32 *>(A.start), rows, static_cast<const u32 *>(A.flag), W.strips, static_cast<const u32 *>(W.len), chars);
}

} // namespace

hipError_t launch_json_wide_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value,
                                  const uint8_t *root_tag, uint32_t rows, uint64_t range_words, uint32_t *offsets, uint8_t *status, void *root_space, void *word_space,
                                  hipStream_t s, const count_total_dev **total) {
  return json_wide_count<false>(tape, string_buf, string_bytes, table, root_value, root_tag, rows, range_words, offsets, status, root_space, word_space, s, total);
}
void launch_json_wide_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                           uint32_t rows, uint64_t range_words, uint8_t *chars, void *root_space, void *word_space, hipStream_t s) {
  json_wide_fill<false>(tape, string_buf, string_bytes, table, root_value, root_tag, rows, range_words, chars, root_space, word_space, s);
}
hipError_t launch_pretty_wide_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value,
                                    const uint8_t *root_tag, uint32_t rows, uint64_t range_words, uint32_t *offsets, uint8_t *status, void *root_space, void *word_space,
                                    hipStream_t s, const count_total_dev **total) {
  return json_wide_count<true>(tape, string_buf, string_bytes, table, root_value, root_tag, rows, range_words, offsets, status, root_space, word_space, s, total);
}
void launch_pretty_wide_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                             uint32_t rows, uint64_t range_words, uint8_t *chars, void *root_space, void *word_space, hipStream_t s) {
  json_wide_fill<true>(tape, string_buf, string_bytes, table, root_value, root_tag, rows, range_words, chars, root_space, word_space, s);
}

} // namespace sjgpu
