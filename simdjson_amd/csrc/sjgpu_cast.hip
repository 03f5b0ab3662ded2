// simdjson_amd/csrc/sjgpu_cast.hip -- typed getters over a column of cells: dom::element::get<T> asked of every cell of a row (sjgpu_cast_cells_device)
// and the census of a row's tags (sjgpu_cell_kinds_device).  Contract: include/sjgpu_cast.h.
//
// Both kernels are elementwise over K rows of n cells (a tag byte and a 64-bit word each) and read neither tape nor string buffer.  The grid is K rows
// of row_blocks workgroups (one dimension, as the query kernels' grids are: row k = blockIdx.x / row_blocks): the row -- and with it the getter -- is uniform
// per workgroup, so the getter's rule is chosen by a scalar branch and no lane dispatches on it.  256 lanes, one per cell, grid-stride over the row in
// steps of 256 cells; a wave's 64 lanes take 64 CONSECUTIVE cells that begin at a multiple of 64: they are one word of the validity bitmap,
// __ballot(code == 0) IS that word and lane 0 stores it.  The loop's bound is the wave's first cell, so the whole wave is in every ballot; a lane beyond n loads and stores nothing and votes 0: the tail bits of a row's last word are 0 by construction.
// Per cell an 8-byte and a 1-byte load, an 8-byte and a 1-byte store, all coalesced; a lane reads its cell before it writes it, so the outputs may be the
// inputs.  The counts are popcounts of ballots kept in wave-uniform registers across the loop, summed over the four waves through LDS, one atomicAdd per
// slot and workgroup into counters the launcher zeroed on the same stream -- no atomic per cell.
// The rules are the reference's (include/simdjson/dom/element-inl.h:219-334; a failed result forwards its code, :60-83); the conversions are the
// compiler's double(int64_t) and double(uint64_t), round to nearest even.
#include "sjgpu_device.h"
#include "sjgpu_cast.h"
#include "sj_cell_kinds.h"

namespace sjgpu {
namespace {

constexpr u32 CAST_THREADS = 256, CAST_WAVES = CAST_THREADS / 64;
constexpr u32 CAST_MAX_WORKGROUPS = 2048; // over all K rows: 8 waves per SIMD of 256 CUs.  More workgroups are more atomics on the same few counters at the kernel's end:
                                          // 10 776 single-step workgroups made the cast of 2.76 M cells 0.10 ms, against 0.015 ms for a copy of its bytes
constexpr u32 E_INCORRECT_TYPE = 17, E_NUMBER_OUT_OF_RANGE = 18, LAST_CODE = 33;
constexpr u64 INT64_TOP = 0x8000000000000000ull;

struct cast_getters {
  u32 packed[CAST_MAX_ROWS / 4]; // getter k: byte k % 4 of word k / 4
};

__device__ __forceinline__ bool is_held_code(u32 t) { return t - 1u < LAST_CODE; }

__device__ __forceinline__ u64 double_bits(double d) {
  u64 b;
  __builtin_memcpy(&b, &d, sizeof b);
  return b;
}

// get<T> of one cell: -> its code, *out = the value (0 with every code but 0).  getter is uniform over the workgroup.
__device__ __forceinline__ u32 cast_cell(u32 getter, u32 t, u64 w, u64 *out) {
  *out = 0;
  if (is_held_code(t)) { return t; }
  bool ok = false, range = false;
  u64 v = w;
  switch (getter) {
    case SJGPU_GET_INT64:
      ok = t == 'l' || (t == 'u' && w < INT64_TOP);
      range = t == 'u';
      break;
    case SJGPU_GET_UINT64:
      ok = t == 'u' || (t == 'l' && w < INT64_TOP);
      range = t == 'l';
      break;
    case SJGPU_GET_DOUBLE:
      ok = t == 'd' || t == 'l' || t == 'u';
      if (t == 'l') { v = double_bits(double(int64_t(w))); }
      if (t == 'u') { v = double_bits(double(w)); }
      break;
    case SJGPU_GET_BOOL:
      ok = t == 't' || t == 'f';
      v = t == 't' ? 1u : 0u;
      break;
    case SJGPU_GET_STRING: ok = t == '"'; break;
    case SJGPU_GET_ARRAY: ok = t == '['; break;
    case SJGPU_GET_OBJECT: ok = t == '{'; break;
    default: break;
  }
  if (ok) {
    *out = v;
    return 0;
  }
  return range ? E_NUMBER_OUT_OF_RANGE : E_INCORRECT_TYPE;
}

// value / tag and value_out / code_out may be the same arrays: no __restrict__ on them
__global__ __launch_bounds__(CAST_THREADS) void k_cast_cells(const u64 *value, const u8 *tag, u32 n, u32 row_blocks, cast_getters getters, u64 *value_out, u8 *code_out,
                                                             u64 *__restrict__ valid_out, u32 *__restrict__ counts) {
  __shared__ u32 s_part[CAST_WAVES][4];
  const u32 k = blockIdx.x / row_blocks, row_block = blockIdx.x - k * row_blocks, lane = lane_id(), wave = threadIdx.x >> 6;
  const u32 getter = (getters.packed[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
  const u64 row = u64(k) * n;
  const u64 *v_in = value + row;
  const u8 *t_in = tag + row;
  u64 *v_out = value_out + row;
  u8 *c_out = code_out + row;
  u64 *valid = valid_out + u64(k) * ((u64(n) + 63u) >> 6);
  u32 c_ok = 0, c_null = 0, c_range = 0, c_held = 0;
  const u64 stride = u64(row_blocks) * CAST_THREADS;
  for (u64 base = u64(row_block) * CAST_THREADS + wave * 64u; base < n; base += stride) { // base: uniform over the wave, a multiple of 64
    const u64 i = base + lane;
    const bool in = i < n;
    u32 t = 0; // (no tag, no code: a lane beyond n counts nowhere)
    u64 w = 0;
    if (in) {
      t = t_in[i];
      w = v_in[i];
    }
    u64 out;
    const u32 code = cast_cell(getter, t, w, &out);
    if (in) {
      v_out[i] = out;
      c_out[i] = u8(code);
    }
    const u64 ok = __ballot(in && code == 0);
    c_ok += u32(__popcll(ok));
    c_null += u32(__popcll(__ballot(t == 'n')));
    c_range += u32(__popcll(__ballot(code == E_NUMBER_OUT_OF_RANGE)));
    c_held += u32(__popcll(__ballot(is_held_code(t))));
    if (lane == 0) { valid[base >> 6] = ok; }
  }
  if (lane == 0) {
    s_part[wave][0] = c_ok;
    s_part[wave][1] = c_null;
    s_part[wave][2] = c_range;
    s_part[wave][3] = c_held;
  }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x < 4) {
    const u32 sum = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
    if (sum) { atomicAdd(&counts[k * 4u + threadIdx.x], sum); }
  }
}

// (the census slots and kind_slot: sj_cell_kinds.h, shared with the census by code of sjgpu_dict.hip)
__global__ __launch_bounds__(CAST_THREADS) void k_cell_kinds(const u64 *__restrict__ value, const u8 *__restrict__ tag, u32 n, u32 row_blocks, u32 *__restrict__ kinds) {
  __shared__ u32 s_part[CAST_WAVES][KIND_SLOTS];
  __shared__ u8 s_slot[256]; // kind_slot of every byte, made once per workgroup (256 lanes, 256 bytes): a table read per cell instead of a divergent switch
  const u32 k = blockIdx.x / row_blocks, row_block = blockIdx.x - k * row_blocks, lane = lane_id(), wave = threadIdx.x >> 6;
  s_slot[threadIdx.x] = u8(kind_slot(threadIdx.x));
  lds_writes_done();
  __syncthreads();
  const u64 row = u64(k) * n;
  const u64 *v_in = value + row;
  const u8 *t_in = tag + row;
  u32 cnt[KIND_NONE];
#pragma unroll
  for (u32 s = 0; s < KIND_NONE; s++) { cnt[s] = 0; }
  const u64 stride = u64(row_blocks) * CAST_THREADS;
  for (u64 base = u64(row_block) * CAST_THREADS + wave * 64u; base < n; base += stride) {
    const u64 i = base + lane;
    u32 slot = KIND_NONE;
    bool negative = false;
    if (i < n) {
      const u32 t = t_in[i];
      const u64 w = v_in[i]; // asked for beside the tag, not behind it (only the l cells need it): a load that waits for the tag is a second latency per step
      slot = s_slot[t];
      negative = t == 'l' && w >= INT64_TOP;
    }
#pragma unroll
    for (u32 s = 0; s < KIND_NONE; s++) { cnt[s] += u32(__popcll(__ballot(s == KIND_NEGATIVE ? negative : slot == s))); }
  }
  if (lane == 0) {
#pragma unroll
    for (u32 s = 0; s < KIND_NONE; s++) { s_part[wave][s] = cnt[s]; }
  }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x < KIND_NONE) {
    const u32 sum = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
    if (sum) { atomicAdd(&kinds[k * KIND_SLOTS + threadIdx.x], sum); }
  }
}

// workgroups per row: one per 256 cells, at most the row's share of CAST_MAX_WORKGROUPS (the rest is the grid-stride loop's)
static inline u32 cast_workgroups(u32 n, u32 K) {
  const u64 all = (u64(n) + CAST_THREADS - 1) / CAST_THREADS, share = CAST_MAX_WORKGROUPS / K;
  return u32(all < share ? all : share);
}

} // namespace

hipError_t launch_cell_kinds(const uint64_t *value, const uint8_t *tag, uint32_t n, uint32_t K, uint32_t *kinds, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(kinds, 0, size_t(K) * KIND_SLOTS * sizeof(u32), s);
  if (e != hipSuccess || n == 0) { return e; }
  const u32 row_blocks = cast_workgroups(n, K);
  hipLaunchKernelGGL(k_cell_kinds, dim3(row_blocks * K), dim3(CAST_THREADS), 0, s, value, tag, n, row_blocks, kinds);
  return hipSuccess;
}

hipError_t launch_cast_cells(const uint64_t *value, const uint8_t *tag, uint32_t n, uint32_t K, const uint8_t *getters, uint64_t *value_out, uint8_t *code_out,
                             uint64_t *valid_out, uint32_t *counts, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(counts, 0, size_t(K) * 4 * sizeof(u32), s);
  if (e != hipSuccess || n == 0) { return e; }
  cast_getters g = {};
  for (u32 k = 0; k < K; k++) { g.packed[k >> 2] |= u32(getters[k]) << (8u * (k & 3u)); }
  const u32 row_blocks = cast_workgroups(n, K);
  hipLaunchKernelGGL(k_cast_cells, dim3(row_blocks * K), dim3(CAST_THREADS), 0, s, value, tag, n, row_blocks, g, value_out, code_out, valid_out, counts);
  return hipSuccess;
}

} // namespace sjgpu
