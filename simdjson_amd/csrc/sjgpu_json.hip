// simdjson_amd/csrc/sjgpu_json.hip -- the JSON text of every cell of one row (sjgpu_serialize_cells_device): simdjson::minify(element) for a batch of elements that
// live on device tapes.  Contract: include/sjgpu_json.h.
//
//   k_rows_locate   (sjgpu_query.hip, shared) what every root is: a container that agrees with the tape and the document it lies in, a scalar, or a code
//   k_json_count    one lane per cell, cells handed out grid-stride: the length of its text and its status.  A container is WALKED, word by word from its opening
//                   word to its closing one, and everything the fill will rely on is decided here: every tag one of the ten, every string record inside its
//                   document's part of the buffer, every number with its second word, every double finite, every closing word of the kind of the level it closes and
//                   pointing back at an opening word that points just behind it, and the walk over exactly at the cell's high index.  Anything else: status 20, length 0.
//   k_gather_total, enqueue_scan   (shared) the lengths' exclusive sum in place and their total in 64 bits
//   k_json_fill     one lane per cell with bytes: the same walk, writing.  It never writes at or beyond offsets[r + 1], whatever the tape says by then.
// The two passes are one template, walk_cell<FILL>.  The only fact of the format that is not local to a tape word is whether a string word is a KEY: it is when the
// innermost open container is an object and its last word was not a key.  That is one bit per nesting level below the cell's root: levels 0 .. 63 are one 64-bit register,
// deeper ones a strip of 63 words per resident lane in the workspace (4 096 levels in all; the parser stops at max_depth <= 4 095), touched only by a push or a pop
// beyond level 63.  The grid is capped at JSON_MAX_WORKGROUPS so that the strips stay at 512 x 256 x 504 bytes = 63 MiB at the most; a call of fewer rows takes less.
// No per-lane array is indexed at run time: digits and escapes go straight to their place in the output (sj_dtoa.h, sj_json_text.h).
// Every loop is bounded by the cell's high - low words, by a string's length or by a number's 20 digits; no lane waits for another.
// PRETTY = true: sjgpu_prettify_cells_device (include/sjgpu_pretty.h), simdjson::prettify(element) -- the same two kernels with the layout of sj_json_walk.h compiled in.
// Cost, not hidden (include/sjgpu_json.h): one lane per cell, a double is converted in both passes, bytes leave one lane at a time.
#include "sjgpu_device.h"
#include "sjgpu_json.h"
#include "sj_json_text.h"
#include "sj_query_program.h"
#include "sj_json_walk.h" // walk_cell<FILL>, serialize_root<FILL>, the sink and the level bits: shared with sjgpu_json_wide.hip

namespace sjgpu {
namespace {

// grid: at most JSON_MAX_WORKGROUPS workgroups; lane = cell, grid-stride.  offsets[r] = the low 32 bits of cell r's length, offsets[rows] = 0, status[r];
// block_sums[workgroup] = the lengths of its cells in 64 bits
template <bool PRETTY>
__global__ __launch_bounds__(JSON_THREADS) void k_json_count(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 string_bytes, const doc_span_dev *__restrict__ table,
                                                             const u64 *__restrict__ root_value, const u8 *__restrict__ root_tag, const u32 *__restrict__ where, u32 rows,
                                                             u64 *__restrict__ strips, u32 *__restrict__ offsets, u8 *__restrict__ status, u64 *__restrict__ block_sums) {
  __shared__ u64 s_sum[JSON_THREADS / 64];
  const u64 lane_global = u64(blockIdx.x) * JSON_THREADS + threadIdx.x, stride = u64(gridDim.x) * JSON_THREADS;
  u64 *strip = strips + lane_global * JSON_STRIP_WORDS;
  u64 sum = 0;
  for (u64 r = lane_global; r < rows; r += stride) {
    json_sink<false> sink = {nullptr, 0, 0};
    const u32 code = serialize_root<false, PRETTY>(tape, sbuf, string_bytes, table, where[r], root_tag[r], root_value[r], strip, sink);
    offsets[r] = u32(sink.at);
    status[r] = u8(code);
    sum += sink.at;
    if (r == 0) { offsets[rows] = 0; } // the scan's last entry: the total lands there
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { sum += __shfl_xor(sum, m); }
  if (lane_id() == 0) { s_sum[threadIdx.x >> 6] = sum; }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) { block_sums[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]; }
}

// the same grid.  The bytes of cell r are chars[offsets[r] .. offsets[r + 1]): only a served cell has any
template <bool PRETTY>
__global__ __launch_bounds__(JSON_THREADS) void k_json_fill(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 string_bytes, const doc_span_dev *__restrict__ table,
                                                            const u64 *__restrict__ root_value, const u8 *__restrict__ root_tag, const u32 *__restrict__ where, u32 rows,
                                                            u64 *__restrict__ strips, const u32 *__restrict__ offsets, u8 *__restrict__ chars) {
  const u64 lane_global = u64(blockIdx.x) * JSON_THREADS + threadIdx.x, stride = u64(gridDim.x) * JSON_THREADS;
  u64 *strip = strips + lane_global * JSON_STRIP_WORDS;
  for (u64 r = lane_global; r < rows; r += stride) {
    const u64 begin = offsets[r], end = offsets[r + 1u];
    if (begin >= end) { continue; }
    json_sink<true> sink = {chars + begin, end - begin, 0};
    (void)serialize_root<true, PRETTY>(tape, sbuf, string_bytes, table, where[r], root_tag[r], root_value[r], strip, sink);
  }
}

static inline u32 json_blocks(u32 rows) {
  const u64 all = (u64(rows) + JSON_THREADS - 1) / JSON_THREADS;
  return u32(all < JSON_MAX_WORKGROUPS ? all : JSON_MAX_WORKGROUPS);
}
static inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// [ctrl, 256 bytes][the count's block sums][the scan's block sums][the lanes' strips]
struct json_workspace {
  count_total_dev *ctrl;
  u64 *block_sums, *strips;
  int *partial;
  size_t bytes;
};
static inline json_workspace carve_json_workspace(void *base, u32 rows) {
  uint8_t *p = static_cast<uint8_t *>(base);
  const u32 blocks = json_blocks(rows);
  json_workspace w;
  size_t at = 0;
  w.ctrl = reinterpret_cast<count_total_dev *>(p + at);  at += 256;
  w.block_sums = reinterpret_cast<u64 *>(p + at);        at += up256(size_t(blocks) * sizeof(u64));
  w.partial = reinterpret_cast<int *>(p + at);           at += up256((size_t((u64(rows) + 1 + 4095) / 4096) + 64) * sizeof(int));
  w.strips = reinterpret_cast<u64 *>(p + at);            at += up256(size_t(blocks) * JSON_THREADS * JSON_STRIP_WORDS * sizeof(u64));
  w.bytes = at;
  return w;
}

template <bool PRETTY>
static const count_total_dev *json_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value,
                                         const uint8_t *root_tag, uint32_t rows, uint32_t *where, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s) {
  const json_workspace w = carve_json_workspace(workspace, rows);
  const u32 blocks = json_blocks(rows);
  launch_rows_locate(tape, table, docs, root_value, root_tag, rows, where, s);
  hipLaunchKernelGGL(k_json_count<PRETTY>, dim3(blocks), dim3(JSON_THREADS), 0, s, tape, string_buf, string_bytes, table, root_value, root_tag, static_cast<const u32 *>(where), rows,
                     w.strips, offsets, status, w.block_sums);
  launch_count_total(w.block_sums, blocks, rows, w.ctrl, s);
  enqueue_scan(reinterpret_cast<int *>(offsets), rows + 1u, &w.ctrl->n_plus_1, w.partial, s);
  return w.ctrl;
}
template <bool PRETTY>
static void json_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                      uint32_t rows, const uint32_t *where, const uint32_t *offsets, uint8_t *chars, void *workspace, hipStream_t s) {
  const json_workspace w = carve_json_workspace(workspace, rows);
  hipLaunchKernelGGL(k_json_fill<PRETTY>, dim3(json_blocks(rows)), dim3(JSON_THREADS), 0, s, tape, string_buf, string_bytes, table, root_value, root_tag, where, rows, w.strips, offsets,
                     chars);
}

} // namespace

size_t json_workspace_bytes(uint32_t rows) { return carve_json_workspace(nullptr, rows).bytes; }

const count_total_dev *launch_json_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value,
                                         const uint8_t *root_tag, uint32_t rows, uint32_t *where, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s) {
  return json_count<false>(tape, string_buf, string_bytes, table, docs, root_value, root_tag, rows, where, offsets, status, workspace, s);
}
void launch_json_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                      uint32_t rows, const uint32_t *where, const uint32_t *offsets, uint8_t *chars, void *workspace, hipStream_t s) {
  json_fill<false>(tape, string_buf, string_bytes, table, root_value, root_tag, rows, where, offsets, chars, workspace, s);
}
const count_total_dev *launch_pretty_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value,
                                           const uint8_t *root_tag, uint32_t rows, uint32_t *where, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s) {
  return json_count<true>(tape, string_buf, string_bytes, table, docs, root_value, root_tag, rows, where, offsets, status, workspace, s);
}
void launch_pretty_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                        uint32_t rows, const uint32_t *where, const uint32_t *offsets, uint8_t *chars, void *workspace, hipStream_t s) {
  json_fill<true>(tape, string_buf, string_bytes, table, root_value, root_tag, rows, where, offsets, chars, workspace, s);
}

} // namespace sjgpu
