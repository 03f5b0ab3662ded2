// simdjson_amd/csrc/sjgpu_write.hip -- typed columns as JSON records (sjgpu_write_records_device): row r of K device-resident columns as the object
// {"key0":v0,"key1":v1,...}, what the reference's builder::string_builder writes for start_object / append_key_value / append_comma / end_object.
// Contract: include/sjgpu_write.h.
//
//   k_write_count   one lane per row, rows handed out grid-stride, the K columns in an inner loop: consecutive lanes read consecutive words of one column.  The row's
//                   length and status, and everything the fill relies on, is decided here: which cells are invalid, and that every string and JSON cell lies inside its
//                   column's characters -- a row with one that does not has status 19 and length 0.  The counts are per-lane sums kept across the loop, added over the
//                   workgroup through shuffles and LDS, one atomicAdd per slot and workgroup into counters the launcher zeroed on the same stream -- no atomic per cell.
//   k_gather_total, enqueue_scan   (shared) the lengths' exclusive sum in place and their total in 64 bits
//   k_write_fill    the same grid.  The 256 rows of one workgroup iteration occupy ONE contiguous span, chars[offsets[r0] .. offsets[r0 + 256)).
//                   Staged road, a span of at most WRITE_WINDOW bytes: every lane writes its row into an LDS window at offsets[r] - offsets[r0], shifted by the
//                   output address's low four bits so that a 16-byte line of the output is a 16-byte line of the window; one barrier; then all 256 lanes copy the
//                   window out in 16-byte stores aligned to the OUTPUT, only the ragged head and tail of the span as bytes.
//                   Direct road, a longer span (one long string among the rows): that iteration's lanes write straight to global memory, as k_json_fill does.
//                   The choice is uniform per workgroup iteration and follows from the offsets alone, so count and fill cannot disagree.  The fill never writes at or
//                   beyond offsets[r + 1], whatever the inputs say by then (text_sink's room), nor outside its window.
//                   There are TWO windows, taken in turn: the barrier of iteration i + 1 stands between the last read of iteration i's window and the first write of
//                   iteration i + 2 into it, so one barrier per iteration is all there is, and no lane waits for another anywhere else.
// The two passes are one template, write_row<FILL>.  No per-lane array is indexed at run time: digits and escapes go straight to their place (sj_dtoa.h, sj_json_text.h).
// Every loop is bounded by K, by a cell's length or by a number's 20 digits.
// -DSJGPU_WRITE_DIRECT_ONLY (a build macro for the lab, scripts/lib_ab.py; never an environment switch) compiles the staged road out.
#include "sjgpu_device.h"
#include "sjgpu_nested.h"
#include "sj_json_text.h"

namespace sjgpu {
namespace {

constexpr u32 WRITE_THREADS = 256;
constexpr u32 WRITE_MAX_WORKGROUPS = 512; // two resident workgroups (their windows) on each of 256 CUs
constexpr u32 WRITE_WINDOW = 28u << 10;   // bytes of one LDS window: 112 per row on average
constexpr u32 WRITE_WINDOW_LINES = WRITE_WINDOW / 16u + 1u; // (+ 1: the span begins up to 15 bytes into its first line)
constexpr u32 LDS_BYTES_PER_CU = 160u << 10;
static_assert(WRITE_WINDOW % 16u == 0, "the window is whole 16-byte lines");
static_assert(2u * (2u * WRITE_WINDOW_LINES * 16u + 256u) <= LDS_BYTES_PER_CU, "two windows per workgroup and at least two workgroups per CU");
static_assert(2u * WRITE_WINDOW_LINES * 16u <= (64u << 10), "what one workgroup may declare");
constexpr u64 LOW32 = 0xFFFFFFFFull;
constexpr u32 E_INDEX_OUT_OF_BOUNDS = 19;

// the text of row r -> its status; the length in sink.at.  *nulls: its invalid cells, *nonfinite: those that are doubles without a text.  Uniform over the
// workgroup: K, the flags, every column's kind -- a lane differs from its neighbour in what its cells hold, never in which code it runs for column k.
// NESTED (k_nested_*; FIELD = write_field_dev): a field may be a LIST -- the same per-value code then runs over the elements list_offsets[r] .. list_offsets[r + 1]
// of the field's column instead of over cell r --, and the flags may ask for an array or a bare value as the row.  *elements, *element_nulls: the elements written,
// those written as null; *nonfinite counts them too.  NESTED = false is the plain writer's instantiation: every statement under NESTED folds away, and its code is
// what it was before there were lists (DESIGN.md 4c-13 has the figures)
__device__ __forceinline__ const write_column_dev &column_of(const write_column_dev &c) { return c; }
__device__ __forceinline__ const write_column_dev &column_of(const write_field_dev &f) { return f.col; }

template <bool FILL, bool NESTED = false, class FIELD = write_column_dev>
__device__ __forceinline__ u32 write_row(const FIELD *__restrict__ cols, const u8 *__restrict__ keys, u32 K, u64 r, u32 flags, text_sink<FILL> &sink, u32 *nulls,
                                         u32 *nonfinite, u32 *elements = nullptr, u32 *element_nulls = nullptr) {
  u32 n_null = 0, n_nonfinite = 0, n_element = 0, n_element_null = 0;
  bool first = true;
  const bool bare = NESTED && (flags & SJGPU_WRITE_BARE) != 0, array = NESTED && (flags & SJGPU_WRITE_ARRAY_ROWS) != 0, keyed = !bare && !array;
  if (!bare) { sink.put(array ? '[' : '{'); }
  for (u32 k = 0; k < K; k++) {
    const FIELD f = cols[k];
    const write_column_dev &c = column_of(f);
    u64 i = r, stop = 0;
    bool in_list = false, first_element = true;
    if constexpr (NESTED) {
      stop = r + 1u;
      if (f.list_offsets != nullptr) {
        const bool list_valid = f.list_valid == nullptr || ((f.list_valid[r >> 6] >> (r & 63u)) & 1u) != 0;
        if (list_valid) { // (the offsets of a list whose validity bit is 0 are not read)
          i = f.list_offsets[r];
          stop = f.list_offsets[r + 1u];
          if (stop < i || stop > f.elements) { return E_INDEX_OUT_OF_BOUNDS; }
        } else {
          n_null++;
          if (flags & SJGPU_WRITE_OMIT_NULLS) { continue; }
        }
        if (!first) { sink.put(','); }
        first = false;
        if (keyed) { sink.put_raw(keys + c.key_at, c.key_len); }
        if (!list_valid) {
          sink.put_null();
          continue;
        }
        sink.put('[');
        in_list = true;
      }
    }
    if (!NESTED || i < stop) {
      do {
        bool valid = c.valid == nullptr || ((c.valid[i >> 6] >> (i & 63u)) & 1u) != 0;
        u64 v = 0, begin = 0, length = 0;
        if (valid) { // (the words of a cell whose validity bit is 0 are not read)
          if (c.values != nullptr) { v = c.values[i]; }
          if (c.kind == SJGPU_COL_STRING || c.kind == SJGPU_COL_JSON) {
            begin = c.offsets[i];
            const u64 end = c.offsets[i + 1u];
            if (end < begin || end > c.chars_bytes) { return E_INDEX_OUT_OF_BOUNDS; }
            length = end - begin;
            valid = c.kind == SJGPU_COL_STRING || length != 0;
          } else if (c.kind == SJGPU_COL_STRING_CELLS) {
            begin = v & LOW32;
            length = v >> 32;
            if (begin + length > c.chars_bytes) { return E_INDEX_OUT_OF_BOUNDS; }
          } else if (c.kind == SJGPU_COL_DOUBLE && !dtoa_is_finite(v)) {
            valid = false;
            n_nonfinite++;
          }
        }
        if (NESTED && in_list) { // an element: a comma of its own level, never a key, never left out
          n_element++;
          n_element_null += valid ? 0u : 1u;
          if (!first_element) { sink.put(','); }
          first_element = false;
        } else {
          if (!valid) {
            n_null++;
            if (flags & SJGPU_WRITE_OMIT_NULLS) { continue; }
          }
          if (!first) { sink.put(','); }
          first = false;
          if (keyed) { sink.put_raw(keys + c.key_at, c.key_len); }
        }
        if (!valid) {
          sink.put_null();
        } else if (c.kind == SJGPU_COL_INT64) {
          sink.put_number(0u, v);
        } else if (c.kind == SJGPU_COL_UINT64) {
          sink.put_number(1u, v);
        } else if (c.kind == SJGPU_COL_DOUBLE) {
          sink.put_number(2u, v);
        } else if (c.kind == SJGPU_COL_BOOL) {
          sink.put_bool(v != 0);
        } else if (c.kind == SJGPU_COL_JSON) {
          sink.put_raw(c.chars + begin, length);
        } else {
          sink.put_string(c.chars + begin, u32(length));
        }
      } while (NESTED && ++i < stop);
    }
    if (NESTED && in_list) { sink.put(']'); }
  }
  if (!bare) { sink.put(array ? ']' : '}'); }
  if ((flags & SJGPU_WRITE_NEWLINE) && !(bare && first)) { sink.put('\n'); } // (a bare row that was left out is empty: no newline either)
  *nulls = n_null;
  *nonfinite = n_nonfinite;
  if constexpr (NESTED) {
    *elements = n_element;
    *element_nulls = n_element_null;
  }
  return 0;
}

// grid: at most WRITE_MAX_WORKGROUPS workgroups; lane = row, grid-stride.  offsets[r] = the low 32 bits of row r's length, offsets[n] = 0, status[r];
// block_sums[workgroup] = the lengths of its rows in 64 bits; counts[0 .. 4) += this workgroup's
__global__ __launch_bounds__(WRITE_THREADS) void k_write_count(const write_column_dev *__restrict__ cols, const u8 *__restrict__ keys, u32 K, u32 n, u32 flags,
                                                               u32 *__restrict__ offsets, u8 *__restrict__ status, u64 *__restrict__ block_sums, u64 *__restrict__ counts) {
  __shared__ u64 s_part[WRITE_THREADS / 64][5];
  const u64 lane_global = u64(blockIdx.x) * WRITE_THREADS + threadIdx.x, stride = u64(gridDim.x) * WRITE_THREADS;
  u64 part[5] = {0, 0, 0, 0, 0}; // the lengths, rows served, rows refused, invalid cells, doubles without a text (indexed by constants only)
  for (u64 r = lane_global; r < n; r += stride) {
    text_sink<false> sink = {nullptr, 0, 0};
    u32 nulls = 0, nonfinite = 0;
    const u32 code = write_row<false>(cols, keys, K, r, flags, sink, &nulls, &nonfinite);
    const u64 length = code ? 0u : sink.at;
    offsets[r] = u32(length);
    status[r] = u8(code);
    part[0] += length;
    part[1] += code ? 0u : 1u;
    part[2] += code ? 1u : 0u;
    part[3] += code ? 0u : nulls;
    part[4] += code ? 0u : nonfinite;
    if (r == 0) { offsets[n] = 0; } // the scan's last entry: the total lands there
  }
#pragma unroll
  for (int j = 0; j < 5; j++) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { part[j] += __shfl_xor(part[j], m); }
  }
  if (lane_id() == 0) {
#pragma unroll
    for (int j = 0; j < 5; j++) { s_part[threadIdx.x >> 6][j] = part[j]; }
  }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x < 5) {
    const u64 sum = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
    if (threadIdx.x == 0) {
      block_sums[blockIdx.x] = sum;
    } else if (sum) {
      atomicAdd(reinterpret_cast<unsigned long long *>(counts) + (threadIdx.x - 1u), static_cast<unsigned long long>(sum));
    }
  }
}

// the same grid.  The bytes of row r are chars[offsets[r] .. offsets[r + 1]): only a served row has any
__global__ __launch_bounds__(WRITE_THREADS) void k_write_fill(const write_column_dev *__restrict__ cols, const u8 *__restrict__ keys, u32 K, u32 n, u32 flags,
                                                              const u32 *__restrict__ offsets, u8 *__restrict__ chars) {
#ifndef SJGPU_WRITE_DIRECT_ONLY
  __shared__ uint4 s_window[2][WRITE_WINDOW_LINES];
  u32 turn = 0;
#endif
  const u64 stride = u64(gridDim.x) * WRITE_THREADS;
  for (u64 r0 = u64(blockIdx.x) * WRITE_THREADS; r0 < n; r0 += stride) { // r0: uniform over the workgroup
    const u64 r = r0 + threadIdx.x, r_end = r0 + WRITE_THREADS < n ? r0 + WRITE_THREADS : u64(n);
    u64 begin = 0, end = 0;
    if (r < n) {
      begin = offsets[r];
      end = offsets[r + 1u];
    }
    u32 nulls, nonfinite;
#ifndef SJGPU_WRITE_DIRECT_ONLY
    const u64 span_begin = offsets[r0], span_end = offsets[r_end];
    const bool staged = span_end >= span_begin && span_end - span_begin <= WRITE_WINDOW; // uniform: from the offsets alone
    if (staged) {
      const u32 span = u32(span_end - span_begin);
      const u32 skew = u32((reinterpret_cast<uintptr_t>(chars) + span_begin) & 15u);
      u8 *const window = reinterpret_cast<u8 *>(s_window[turn]);
      if (begin < end && begin >= span_begin && end <= span_end) {
        text_sink<true> sink = {window + skew + (begin - span_begin), end - begin, 0};
        (void)write_row<true>(cols, keys, K, r, flags, sink, &nulls, &nonfinite);
      }
      lds_writes_done();
      __syncthreads();
      // line c of the window is the 16 bytes of the output at chars + span_begin - skew + 16 c
      const u32 lines = (skew + span + 15u) >> 4, last = skew + span;
      for (u32 c = threadIdx.x; c < lines; c += WRITE_THREADS) {
        const u32 lo = c << 4;
        if (lo >= skew && lo + 16u <= last) {
          *reinterpret_cast<uint4 *>(chars + (span_begin + lo - skew)) = s_window[turn][c];
        } else {
          for (u32 p = lo < skew ? skew : lo; p < lo + 16u && p < last; p++) { chars[span_begin + p - skew] = window[p]; }
        }
      }
    } else {
      if (begin < end) {
        text_sink<true> sink = {chars + begin, end - begin, 0};
        (void)write_row<true>(cols, keys, K, r, flags, sink, &nulls, &nonfinite);
      }
      lds_writes_done();
      __syncthreads(); // (every iteration has its barrier: the turn of the windows stands on it)
    }
    turn ^= 1u;
#else
    (void)r_end;
    if (begin < end) {
      text_sink<true> sink = {chars + begin, end - begin, 0};
      (void)write_row<true>(cols, keys, K, r, flags, sink, &nulls, &nonfinite);
    }
#endif
  }
}

// ---- list columns and array rows (sjgpu_write_nested_device, include/sjgpu_nested.h): the same two passes over write_row<FILL, true> -----------------------
// k_nested_count: k_write_count with two more sums, the elements written and those written as null: counts[0 .. 6)
__global__ __launch_bounds__(WRITE_THREADS) void k_nested_count(const write_field_dev *__restrict__ fields, const u8 *__restrict__ keys, u32 K, u32 n, u32 flags,
                                                                u32 *__restrict__ offsets, u8 *__restrict__ status, u64 *__restrict__ block_sums, u64 *__restrict__ counts) {
  __shared__ u64 s_part[WRITE_THREADS / 64][7];
  const u64 lane_global = u64(blockIdx.x) * WRITE_THREADS + threadIdx.x, stride = u64(gridDim.x) * WRITE_THREADS;
  u64 part[7] = {0, 0, 0, 0, 0, 0, 0}; // the lengths, rows served, rows refused, invalid fields, doubles without a text, elements, null elements (constants only)
  for (u64 r = lane_global; r < n; r += stride) {
    text_sink<false> sink = {nullptr, 0, 0};
    u32 nulls = 0, nonfinite = 0, elements = 0, element_nulls = 0;
    const u32 code = write_row<false, true>(fields, keys, K, r, flags, sink, &nulls, &nonfinite, &elements, &element_nulls);
    const u64 length = code ? 0u : sink.at;
    offsets[r] = u32(length);
    status[r] = u8(code);
    part[0] += length;
    part[1] += code ? 0u : 1u;
    part[2] += code ? 1u : 0u;
    part[3] += code ? 0u : nulls;
    part[4] += code ? 0u : nonfinite;
    part[5] += code ? 0u : elements;
    part[6] += code ? 0u : element_nulls;
    if (r == 0) { offsets[n] = 0; } // the scan's last entry: the total lands there
  }
#pragma unroll
  for (int j = 0; j < 7; j++) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { part[j] += __shfl_xor(part[j], m); }
  }
  if (lane_id() == 0) {
#pragma unroll
    for (int j = 0; j < 7; j++) { s_part[threadIdx.x >> 6][j] = part[j]; }
  }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x < 7) {
    const u64 sum = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
    if (threadIdx.x == 0) {
      block_sums[blockIdx.x] = sum;
    } else if (sum) {
      atomicAdd(reinterpret_cast<unsigned long long *>(counts) + (threadIdx.x - 1u), static_cast<unsigned long long>(sum));
    }
  }
}

// Whether a run of rows whose texts are chars[a .. b) fits one window
__device__ __forceinline__ bool fits_window(u64 a, u64 b) { return b >= a && b - a <= WRITE_WINDOW; }

// k_nested_fill: k_write_fill's grid and its two roads over write_row<true, true>: the 256 rows of an iteration go through an LDS window when their span fits it
// and straight to chars when it does not; which follows from nine of the offsets -- the same words for every lane --, so it is uniform over the workgroup and
// count and fill cannot disagree; a lane whose offsets do not lie inside the span writes nothing.  Each window use has one barrier and flips the turn, and nothing
// else does: the barrier of use u + 1 stands between the last read of use u's window and the first write of use u + 2 into it.  The barrier guards LDS only (the
// drained bytes are nobody's to read), so it does not wait for the drain's global stores.
// With lists a row is several times longer and 256 rows often do not fit.  -DSJGPU_NESTED_SPLIT (a build macro for the lab, as SJGPU_WRITE_DIRECT_ONLY, which holds
// here too; never an environment switch) compiles the SPLIT in: such an iteration is cut into equal groups of 128, 64 or 32 consecutive rows -- the largest size for
// which EVERY group's span fits -- and the groups go through the two windows in turn: the group's lanes write their rows, one barrier, all 256 lanes drain.  It is
// NOT in the product: measured (profiles/nested_write.txt), the split lost to the direct road on every leg it applied to -- 2.3 x slower with
// 64-row groups, where one wave writes while three wait at the barrier -- so the product goes direct whenever 256 rows do not fit.
__global__ __launch_bounds__(WRITE_THREADS) void k_nested_fill(const write_field_dev *__restrict__ fields, const u8 *__restrict__ keys, u32 K, u32 n, u32 flags,
                                                               const u32 *__restrict__ offsets, u8 *__restrict__ chars) {
#ifndef SJGPU_WRITE_DIRECT_ONLY
  __shared__ uint4 s_window[2][WRITE_WINDOW_LINES];
  u32 turn = 0;
#endif
  const u64 stride = u64(gridDim.x) * WRITE_THREADS;
  for (u64 r0 = u64(blockIdx.x) * WRITE_THREADS; r0 < n; r0 += stride) { // r0: uniform over the workgroup
    const u64 r = r0 + threadIdx.x, r_end = r0 + WRITE_THREADS < n ? r0 + WRITE_THREADS : u64(n);
    u64 begin = 0, end = 0;
    if (r < n) {
      begin = offsets[r];
      end = offsets[r + 1u];
    }
    u32 nulls, nonfinite, elements, element_nulls;
    u32 group = 0; // the rows of one window use; 0: the direct road
#ifndef SJGPU_WRITE_DIRECT_ONLY
    {
      const auto edge = [&](u32 j) -> u64 { return offsets[r0 + 32u * j < r_end ? r0 + 32u * j : r_end]; };
      const u64 e0 = edge(0), e8 = edge(8);
      if (fits_window(e0, e8)) {
        group = 256u;
      }
#ifdef SJGPU_NESTED_SPLIT
      else {
        const u64 e1 = edge(1), e2 = edge(2), e3 = edge(3), e4 = edge(4), e5 = edge(5), e6 = edge(6), e7 = edge(7);
        if (fits_window(e0, e4) && fits_window(e4, e8)) {
          group = 128u;
        } else if (fits_window(e0, e2) && fits_window(e2, e4) && fits_window(e4, e6) && fits_window(e6, e8)) {
          group = 64u;
        } else if (fits_window(e0, e1) && fits_window(e1, e2) && fits_window(e2, e3) && fits_window(e3, e4) && fits_window(e4, e5) && fits_window(e5, e6) &&
                   fits_window(e6, e7) && fits_window(e7, e8)) {
          group = 32u;
        }
      }
#endif
    }
    for (u32 g = 0; group != 0u && g < WRITE_THREADS && r0 + g < r_end; g += group) { // g, the group's edges and its span: uniform
      const u64 g_end = r0 + g + group < r_end ? r0 + g + group : r_end;
      const u64 span_begin = offsets[r0 + g], span_end = offsets[g_end];
      if (!fits_window(span_begin, span_end) || span_end == span_begin) { continue; } // (nothing to write; a span that does not fit cannot be, the edges said so)
      const u32 span = u32(span_end - span_begin);
      const u32 skew = u32((reinterpret_cast<uintptr_t>(chars) + span_begin) & 15u);
      u8 *const window = reinterpret_cast<u8 *>(s_window[turn]);
      if (threadIdx.x >= g && threadIdx.x < g + group && begin < end && begin >= span_begin && end <= span_end) {
        text_sink<true> sink = {window + skew + (begin - span_begin), end - begin, 0};
        (void)write_row<true, true>(fields, keys, K, r, flags, sink, &nulls, &nonfinite, &elements, &element_nulls);
      }
      lds_writes_done();
      workgroup_barrier_lds_only();
      // line c of the window is the 16 bytes of the output at chars + span_begin - skew + 16 c
      const u32 lines = (skew + span + 15u) >> 4, last = skew + span;
      for (u32 c = threadIdx.x; c < lines; c += WRITE_THREADS) {
        const u32 lo = c << 4;
        if (lo >= skew && lo + 16u <= last) {
          *reinterpret_cast<uint4 *>(chars + (span_begin + lo - skew)) = s_window[turn][c];
        } else {
          for (u32 p = lo < skew ? skew : lo; p < lo + 16u && p < last; p++) { chars[span_begin + p - skew] = window[p]; }
        }
      }
      turn ^= 1u;
    }
#endif
    if (group == 0u && begin < end) {
      text_sink<true> sink = {chars + begin, end - begin, 0};
      (void)write_row<true, true>(fields, keys, K, r, flags, sink, &nulls, &nonfinite, &elements, &element_nulls);
    }
  }
}

static inline u32 write_blocks(u32 n) {
  const u64 all = (u64(n) + WRITE_THREADS - 1) / WRITE_THREADS;
  return u32(all < WRITE_MAX_WORKGROUPS ? all : WRITE_MAX_WORKGROUPS);
}
static inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// [ctrl, 256 bytes][the count's block sums][the scan's block sums]
struct write_workspace {
  count_total_dev *ctrl;
  u64 *block_sums;
  int *partial;
  size_t bytes;
};
static inline write_workspace carve_write_workspace(void *base, u32 n) {
  uint8_t *p = static_cast<uint8_t *>(base);
  write_workspace w;
  size_t at = 0;
  w.ctrl = reinterpret_cast<count_total_dev *>(p + at);  at += 256;
  w.block_sums = reinterpret_cast<u64 *>(p + at);        at += up256(size_t(write_blocks(n)) * sizeof(u64));
  w.partial = reinterpret_cast<int *>(p + at);           at += up256((size_t((u64(n) + 1 + 4095) / 4096) + 64) * sizeof(int));
  w.bytes = at;
  return w;
}

} // namespace

size_t write_workspace_bytes(uint32_t n) { return carve_write_workspace(nullptr, n).bytes; }
uint32_t write_rows_per_step() { return WRITE_THREADS; }
uint32_t write_max_workgroups() { return WRITE_MAX_WORKGROUPS; }
uint32_t write_window_bytes() { return WRITE_WINDOW; }

const count_total_dev *launch_write_count(const write_column_dev *cols, const uint8_t *keys, uint32_t K, uint32_t n, uint32_t flags, uint32_t *offsets, uint8_t *status,
                                          uint64_t *counts, void *workspace, hipStream_t s) {
  const write_workspace w = carve_write_workspace(workspace, n);
  const u32 blocks = write_blocks(n);
  (void)hipMemsetAsync(counts, 0, 4 * sizeof(u64), s);
  hipLaunchKernelGGL(k_write_count, dim3(blocks), dim3(WRITE_THREADS), 0, s, cols, keys, K, n, flags, offsets, status, w.block_sums, counts);
  launch_count_total(w.block_sums, blocks, n, w.ctrl, s);
  enqueue_scan(reinterpret_cast<int *>(offsets), n + 1u, &w.ctrl->n_plus_1, w.partial, s);
  return w.ctrl;
}

void launch_write_fill(const write_column_dev *cols, const uint8_t *keys, uint32_t K, uint32_t n, uint32_t flags, const uint32_t *offsets, uint8_t *chars, hipStream_t s) {
  hipLaunchKernelGGL(k_write_fill, dim3(write_blocks(n)), dim3(WRITE_THREADS), 0, s, cols, keys, K, n, flags, offsets, chars);
}

const count_total_dev *launch_nested_count(const write_field_dev *fields, const uint8_t *keys, uint32_t K, uint32_t n, uint32_t flags, uint32_t *offsets, uint8_t *status,
                                           uint64_t *counts, void *workspace, hipStream_t s) {
  const write_workspace w = carve_write_workspace(workspace, n);
  const u32 blocks = write_blocks(n);
  (void)hipMemsetAsync(counts, 0, 6 * sizeof(u64), s);
  hipLaunchKernelGGL(k_nested_count, dim3(blocks), dim3(WRITE_THREADS), 0, s, fields, keys, K, n, flags, offsets, status, w.block_sums, counts);
  launch_count_total(w.block_sums, blocks, n, w.ctrl, s);
  enqueue_scan(reinterpret_cast<int *>(offsets), n + 1u, &w.ctrl->n_plus_1, w.partial, s);
  return w.ctrl;
}

void launch_nested_fill(const write_field_dev *fields, const uint8_t *keys, uint32_t K, uint32_t n, uint32_t flags, const uint32_t *offsets, uint8_t *chars, hipStream_t s) {
  hipLaunchKernelGGL(k_nested_fill, dim3(write_blocks(n)), dim3(WRITE_THREADS), 0, s, fields, keys, K, n, flags, offsets, chars);
}

} // namespace sjgpu
