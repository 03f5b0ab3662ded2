// simdjson_amd/csrc/sjgpu_pivot.hip -- a map column pivoted into a record table (sjgpu_pivot_fields_device).  Contract: include/sjgpu_pivot.h.
//
// The call reads the fields' offsets, statuses, value row and tag row, the codes of their keys and, when there is one, the map from codes to columns; no tape,
// no string buffer, no workspace.  Cell (c, r) lies at c * rows + r of both outputs.
//   k_pivot_fill      every cell's default: tag = its row's status, or 20 (NO_SUCH_FIELD) where that is 0; value 0.  One lane per FOUR consecutive cells: two
//                     16-byte stores for the words and one 4-byte store for the tags (gfx950 stores a dword at any byte address).  The words begin at an 8-byte
//                     aligned address: when that is no 16-byte one, cell 0 is lane 0's extra and the groups of four begin at cell 1.  What is left at the end
//                     (fewer than four cells) is stored cell by cell.
//   k_pivot_scatter   behind it on the stream: one lane per row, consecutive lanes on consecutive rows.  A row whose status is not 0, whose slice runs backwards
//                     or ends beyond `fields` is left as the fill made it, and none of its slots is read.  Else the lane takes its slots from the LAST to the
//                     FIRST and stores each slot that has a column at its cell: the first field of the row that maps to a column is the last store to that cell,
//                     and a lane's own stores to one address stay in program order.  No atomics: nothing here depends on which lane or which workgroup ran first.
// One lane per row: a row of a million fields is ONE lane's work (include/sjgpu_pivot.h, "Cost, not hidden").
#include "sjgpu_device.h"
#include "sjgpu_pivot.h"

namespace sjgpu {
namespace {

constexpr u32 PIVOT_THREADS = 256;
constexpr u32 PIVOT_FILL_CELLS = 4; // per lane
constexpr u8 PIVOT_NO_SUCH_FIELD = 20;

typedef u64 u64x2 __attribute__((vector_size(16)));
typedef u32 __attribute__((aligned(1))) u32_any;

__device__ __forceinline__ u32 default_tag(const u8 *__restrict__ status, u32 r) {
  const u32 st = status[r];
  return st ? st : PIVOT_NO_SUCH_FIELD;
}

// head: 1 when value_out is 8 bytes past a 16-byte address (cell 0 is stored alone), else 0
__global__ __launch_bounds__(PIVOT_THREADS) void k_pivot_fill(const u8 *__restrict__ status, u32 rows, u64 cells, u32 head, u64 *__restrict__ value_out,
                                                             u8 *__restrict__ tag_out) {
  const u64 j = u64(blockIdx.x) * PIVOT_THREADS + threadIdx.x;
  if (j == 0 && head) {
    value_out[0] = 0;
    tag_out[0] = u8(default_tag(status, 0));
  }
  const u64 c0 = head + PIVOT_FILL_CELLS * j;
  if (c0 >= cells) { return; }
  u32 r = u32(c0 % rows);
  if (c0 + PIVOT_FILL_CELLS <= cells) {
    u32 tags = 0;
#pragma unroll
    for (u32 k = 0; k < PIVOT_FILL_CELLS; k++) {
      tags |= default_tag(status, r) << (8u * k);
      r = r + 1u == rows ? 0u : r + 1u;
    }
    u64x2 *const words = reinterpret_cast<u64x2 *>(value_out + c0); // (16-byte aligned: c0 - head is a multiple of four, and `head` is what value_out lacks)
    const u64x2 zero = {0, 0};
    words[0] = zero;
    words[1] = zero;
    *reinterpret_cast<u32_any *>(tag_out + c0) = tags;
    return;
  }
  for (u64 c = c0; c < cells; c++) {
    value_out[c] = 0;
    tag_out[c] = u8(default_tag(status, r));
    r = r + 1u == rows ? 0u : r + 1u;
  }
}

__global__ __launch_bounds__(PIVOT_THREADS) void k_pivot_scatter(const u32 *__restrict__ offsets, const u8 *__restrict__ status, u32 rows, const int *__restrict__ codes,
                                                                const u64 *__restrict__ value, const u8 *__restrict__ tag, u32 fields,
                                                                const int *__restrict__ column_of_code, u32 groups, u32 columns, u64 *value_out, u8 *tag_out) {
  const u64 r = u64(blockIdx.x) * PIVOT_THREADS + threadIdx.x;
  if (r >= rows || status[r]) { return; }
  const u32 lo = offsets[r], hi = offsets[r + 1];
  if (lo > hi || hi > fields) { return; }
  for (u32 i = hi; i-- > lo;) {
    const u32 code = u32(codes[i]); // (-1 and every other negative code: beyond any groups)
    if (code >= groups) { continue; }
    const u32 column = column_of_code ? u32(column_of_code[code]) : code;
    if (column >= columns) { continue; }
    const u64 at = u64(column) * rows + r;
    value_out[at] = value[i];
    tag_out[at] = tag[i];
  }
}

static inline u32 pivot_blocks(u64 n) { return u32((n + PIVOT_THREADS - 1) / PIVOT_THREADS); }

} // namespace

void launch_pivot_fields(const uint32_t *offsets, const uint8_t *status, uint32_t rows, const int32_t *codes, const uint64_t *value, const uint8_t *tag, uint32_t fields,
                         const int32_t *column_of_code, uint32_t groups, uint32_t columns, uint64_t *value_out, uint8_t *tag_out, hipStream_t s) {
  const u64 cells = u64(columns) * rows; // 1 .. PIVOT_MAX_CELLS
  const u32 head = u32((reinterpret_cast<uintptr_t>(value_out) >> 3) & 1u);
  const u64 fill_lanes = cells / PIVOT_FILL_CELLS + 1; // (covers cells - head in fours, rounded up, and is never 0)
  hipLaunchKernelGGL(k_pivot_fill, dim3(pivot_blocks(fill_lanes)), dim3(PIVOT_THREADS), 0, s, status, rows, cells, head, value_out, tag_out);
  hipLaunchKernelGGL(k_pivot_scatter, dim3(pivot_blocks(rows)), dim3(PIVOT_THREADS), 0, s, offsets, status, rows, codes, value, tag, fields, column_of_code, groups, columns,
                     value_out, tag_out);
}

} // namespace sjgpu
