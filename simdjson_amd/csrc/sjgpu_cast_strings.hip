// simdjson_amd/csrc/sjgpu_cast_strings.hip -- numbers held in strings: get_int64_in_string, get_uint64_in_string and get_double_in_string asked of every cell
// of a row (sjgpu_cast_string_cells_device).  Contract: include/sjgpu_cast_strings.h; the rules: sj_number_in_string.h.
//
// k_cast_string_cells has the grid and the bookkeeping of k_cast_cells (sjgpu_cast.hip): K rows of row_blocks workgroups, the getter uniform per workgroup, 256
// lanes, a lane per cell, grid-stride; a wave's 64 consecutive cells are one word of the validity bitmap and __ballot(code == 0) is that word; the counts are
// popcounts of ballots, summed over the four waves through LDS, one atomicAdd per slot and workgroup.
// What is new: a `"` cell's lane reads its string where it lies in the string buffer -- the first WINDOW = 32 bytes from the string's first byte on, as one or
// two 16-byte loads at whatever alignment the string has (the hardware serves them; nothing in FRONT of the string is touched), byte by byte only for the strings
// that begin within 32 bytes of the buffer's end -- and parses it out of those four 64-bit registers: string_window::byte is a select and a shift, there is no
// array a lane indexes and so no scratch memory.  Either integer rule needs 22 bytes at the most (sj_number_in_string.h), so every integer getter is settled
// here, and so is every double of at most 19 significant digits whose string fits the window (decimal_to_binary64).
// A double cell that does not -- more than 19 significant digits, or more than 32 bytes -- is PARKED: PARKED goes into code_out (no code and no tag a finished
// call leaves: the codes are 0, 9, 17, 18 and what a cell held, 1 .. 33), the value word is not written (in place it still is the cell's offset and length),
// the cell votes 0 in the ballot and slot [5] counts it.  k_cast_strings_exact is always enqueued behind: it reads [5] of its row and leaves at once when that
// is 0; otherwise it looks for the markers, decides each such cell from the bytes in memory with decide_long_decimal (two big integers per lane, in LDS: neither
// kernel has scratch), writes value and code, sets the validity bit with an atomic OR into the word the first kernel stored
// and adds to [0] or [2].  No workspace, no list, no capacity, no read-back; no marker survives the call.
#include "sjgpu_device.h"
#include "sjgpu_cast_strings.h"
#include "sj_number_in_string.h"

namespace sjgpu {
namespace {

constexpr u32 GETS_THREADS = 256, GETS_WAVES = GETS_THREADS / 64, GETS_EXACT_THREADS = 64;
constexpr u32 GETS_MAX_WORKGROUPS = 2048; // over all K rows, as CAST_MAX_WORKGROUPS of sjgpu_cast.hip and for its reason: the atomics on the same few counters
constexpr u32 E_INCORRECT_TYPE = 17, E_NUMBER_OUT_OF_RANGE = 18, LAST_CODE = 33;
constexpr u32 PARKED = 0xFFu;
constexpr u32 WINDOW = 32;
constexpr u64 INT64_TOP = 0x8000000000000000ull, LOW32 = 0xFFFFFFFFull;
enum : u32 { SLOT_OK = 0, SLOT_NULL = 1, SLOT_NUMBER_ERROR = 2, SLOT_HELD = 3, SLOT_REFUSED = 4, SLOT_EXACT = 5, SLOT_OUTSIDE = 6, SLOTS = 8 };

struct gets_getters {
  u32 packed[CAST_MAX_ROWS / 4]; // getter k: byte k % 4 of word k / 4
};

__device__ __forceinline__ bool is_held_code(u32 t) { return t - 1u < LAST_CODE; }

__device__ __forceinline__ u64 double_bits(double d) {
  u64 b;
  __builtin_memcpy(&b, &d, sizeof b);
  return b;
}

// the first WINDOW bytes of a string in four registers
struct string_window {
  u64 a, b, c, d;
  __device__ __forceinline__ u32 byte(u32 p) const {
    const u64 wa = a, wb = b, wc = c, wd = d; // four values, then selects: a select between the MEMBERS is a dynamic address, and the window becomes an array
    const u64 lo = p < 8u ? wa : wb, hi = p < 24u ? wc : wd;
    return u32((p < 16u ? lo : hi) >> (8u * (p & 7u))) & 0xFFu;
  }
};
struct u64x2 { u64 lo, hi; };
__device__ __forceinline__ u64x2 load16_any(const u8 *p) { // 16 bytes at any alignment
  u64x2 v;
  __builtin_memcpy(&v, p, sizeof v);
  return v;
}
// s[0 .. take) and whatever follows it INSIDE the buffer; room = the bytes from s to the buffer's end (>= take)
__device__ __forceinline__ string_window load_window(const u8 *s, u32 take, u64 room) {
  string_window w{0, 0, 0, 0};
  u32 have = 0;
  if (room >= 16u) {
    const u64x2 v = load16_any(s);
    w.a = v.lo;
    w.b = v.hi;
    have = 16;
    if (take > 16u && room >= 32u) {
      const u64x2 x = load16_any(s + 16);
      w.c = x.lo;
      w.d = x.hi;
      have = 32;
    }
  }
#pragma unroll 1
  for (u32 j = have; j < take; j++) { // a string that begins within 32 bytes of the buffer's end
    const u64 v = u64(s[j]) << (8u * (j & 7u));
    const u32 q = j >> 3;
    w.a |= q == 0u ? v : 0;
    w.b |= q == 1u ? v : 0;
    w.c |= q == 2u ? v : 0;
    w.d |= q == 3u ? v : 0;
  }
  return w;
}

struct memory_bytes {
  const u8 *p;
  __device__ __forceinline__ u32 byte(u32 i) const { return p[i]; }
};

// get<T> of a number cell (SJGPU_GETS_OR_NUMBER): the rule of sjgpu_cast.hip's cast_cell for the three number getters, -> the code
__device__ __forceinline__ u32 number_cell(u32 getter, u32 t, u64 w, u64 *out) {
  bool ok = false, range = false;
  u64 v = w;
  if (getter == SJGPU_GETS_INT64) {
    ok = t == 'l' || (t == 'u' && w < INT64_TOP);
    range = t == 'u';
  } else if (getter == SJGPU_GETS_UINT64) {
    ok = t == 'u' || (t == 'l' && w < INT64_TOP);
    range = t == 'l';
  } else {
    ok = t == 'd' || t == 'l' || t == 'u';
    if (t == 'l') { v = double_bits(double(int64_t(w))); }
    if (t == 'u') { v = double_bits(double(w)); }
  }
  if (ok) {
    *out = v;
    return 0;
  }
  return range ? E_NUMBER_OUT_OF_RANGE : E_INCORRECT_TYPE;
}

// value / tag and value_out / code_out may be the same arrays: no __restrict__ on them
__global__ __launch_bounds__(GETS_THREADS) void k_cast_string_cells(const u8 *__restrict__ sbuf, u64 string_bytes, const u64 *value, const u8 *tag, u32 n, u32 row_blocks,
                                                                    gets_getters getters, u64 *value_out, u8 *code_out, u64 *__restrict__ valid_out, u32 *__restrict__ counts) {
  __shared__ u32 s_part[GETS_WAVES][SLOTS];
  const u32 k = blockIdx.x / row_blocks, row_block = blockIdx.x - k * row_blocks, lane = lane_id(), wave = threadIdx.x >> 6;
  const u32 getter_byte = (getters.packed[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
  const u32 getter = getter_byte & 0xFu;
  const bool or_number = (getter_byte & SJGPU_GETS_OR_NUMBER) != 0u;
  const u64 row = u64(k) * n;
  const u64 *v_in = value + row;
  const u8 *t_in = tag + row;
  u64 *v_out = value_out + row;
  u8 *c_out = code_out + row;
  u64 *valid = valid_out + u64(k) * ((u64(n) + 63u) >> 6);
  u32 c_ok = 0, c_null = 0, c_error = 0, c_held = 0, c_refused = 0, c_parked = 0, c_outside = 0;
  const u64 stride = u64(row_blocks) * GETS_THREADS;
  for (u64 base = u64(row_block) * GETS_THREADS + wave * 64u; base < n; base += stride) { // base: uniform over the wave, a multiple of 64
    const u64 i = base + lane;
    const bool in = i < n;
    u32 t = 0; // (no tag, no code: a lane beyond n counts nowhere)
    u64 w = 0;
    if (in) {
      t = t_in[i];
      w = v_in[i];
    }
    u64 out = 0;
    u32 code = E_INCORRECT_TYPE;
    bool refused = false, parked = false, outside = false;
    if (is_held_code(t)) {
      code = t;
    } else if (t == '"') {
      const u64 off = w & LOW32;
      const u32 len = u32(w >> 32);
      if (off + len > string_bytes) {
        outside = true;
      } else if (getter == SJGPU_GETS_DOUBLE && len > WINDOW) {
        parked = true;
      } else {
        const string_window win = load_window(sbuf + off, len < WINDOW ? len : WINDOW, string_bytes - off);
        in_string_number r;
        if (getter == SJGPU_GETS_DOUBLE) { r = parse_double_in_string<false>(win, len, static_cast<bigint *>(nullptr)); }
        else { r = parse_integer_in_string(win, len, getter == SJGPU_GETS_UINT64); }
        parked = r.slow;
        code = r.code;
        out = r.code ? 0 : r.value;
      }
    } else if (or_number && (t == 'l' || t == 'u' || t == 'd')) {
      code = number_cell(getter, t, w, &out);
    } else {
      refused = in;
    }
    if (in) {
      if (parked) {
        c_out[i] = u8(PARKED);
      } else {
        v_out[i] = out;
        c_out[i] = u8(code);
      }
    }
    const u64 ok = __ballot(in && !parked && code == 0);
    c_ok += u32(__popcll(ok));
    c_null += u32(__popcll(__ballot(t == 'n')));
    c_error += u32(__popcll(__ballot(!parked && code == SJ_NUMBER_ERROR)));
    c_held += u32(__popcll(__ballot(is_held_code(t))));
    c_refused += u32(__popcll(__ballot(refused)));
    c_parked += u32(__popcll(__ballot(parked)));
    c_outside += u32(__popcll(__ballot(outside)));
    if (lane == 0) { valid[base >> 6] = ok; }
  }
  if (lane == 0) {
    s_part[wave][SLOT_OK] = c_ok;
    s_part[wave][SLOT_NULL] = c_null;
    s_part[wave][SLOT_NUMBER_ERROR] = c_error;
    s_part[wave][SLOT_HELD] = c_held;
    s_part[wave][SLOT_REFUSED] = c_refused;
    s_part[wave][SLOT_EXACT] = c_parked;
    s_part[wave][SLOT_OUTSIDE] = c_outside;
    s_part[wave][7] = 0;
  }
  lds_writes_done();
  __syncthreads();
  if (threadIdx.x < SLOTS) {
    const u32 sum = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
    if (sum) { atomicAdd(&counts[k * SLOTS + threadIdx.x], sum); }
  }
}

// the parked cells of the rows that have any: value (the input row) still holds their words, code_out their markers
__global__ __launch_bounds__(GETS_EXACT_THREADS) void k_cast_strings_exact(const u8 *__restrict__ sbuf, const u64 *value, u32 n, u32 row_blocks, u64 *value_out, u8 *code_out,
                                                                           u64 *valid_out, u32 *counts) {
  // two big integers of 516 bytes per lane, in LDS: 64.5 KiB per workgroup of one wave (gfx950 has 160 KiB per CU), a lane's pair 129 words from its neighbour's,
  // so the lanes of a wave that walk their integers in step meet no bank twice.  No kernel of this file uses private memory.
  __shared__ bigint s_big[GETS_EXACT_THREADS][2];
  const u32 k = blockIdx.x / row_blocks, row_block = blockIdx.x - k * row_blocks;
  if (counts[k * SLOTS + SLOT_EXACT] == 0) { return; } // (written by the kernel in front; this kernel adds to [0] and [2] only)
  const u64 row = u64(k) * n;
  const u64 *v_in = value + row;
  u64 *v_out = value_out + row;
  u8 *c_out = code_out + row;
  u64 *valid = valid_out + u64(k) * ((u64(n) + 63u) >> 6);
  bigint *big = s_big[threadIdx.x];
  const u64 stride = u64(row_blocks) * GETS_EXACT_THREADS;
  for (u64 i = u64(row_block) * GETS_EXACT_THREADS + threadIdx.x; i < n; i += stride) {
    if (c_out[i] != PARKED) { continue; }
    const u64 w = v_in[i];
    const memory_bytes src{sbuf + (w & LOW32)};
    const in_string_number r = parse_double_in_string<true>(src, u32(w >> 32), big);
    v_out[i] = r.code ? 0 : r.value;
    c_out[i] = u8(r.code);
    if (r.code == 0) {
      atomicOr(reinterpret_cast<unsigned long long *>(valid + (i >> 6)), (unsigned long long)(1ull << (i & 63u)));
      atomicAdd(&counts[k * SLOTS + SLOT_OK], 1u);
    } else if (r.code == SJ_NUMBER_ERROR) {
      atomicAdd(&counts[k * SLOTS + SLOT_NUMBER_ERROR], 1u);
    }
  }
}

// workgroups per row: one per `threads` cells, at most the row's share of GETS_MAX_WORKGROUPS (the rest is the grid-stride loop's)
static inline u32 gets_workgroups(u32 n, u32 K, u32 threads) {
  const u64 all = (u64(n) + threads - 1) / threads, share = GETS_MAX_WORKGROUPS / K;
  return u32(all < share ? all : share);
}

} // namespace

hipError_t launch_cast_string_cells(const uint8_t *string_buf, uint64_t string_bytes, const uint64_t *value, const uint8_t *tag, uint32_t n, uint32_t K, const uint8_t *getters,
                                    uint64_t *value_out, uint8_t *code_out, uint64_t *valid_out, uint32_t *counts, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(counts, 0, size_t(K) * SLOTS * sizeof(u32), s);
  if (e != hipSuccess || n == 0) { return e; }
  gets_getters g = {};
  for (u32 k = 0; k < K; k++) { g.packed[k >> 2] |= u32(getters[k]) << (8u * (k & 3u)); }
  const u32 row_blocks = gets_workgroups(n, K, GETS_THREADS), exact_blocks = gets_workgroups(n, K, GETS_EXACT_THREADS);
  hipLaunchKernelGGL(k_cast_string_cells, dim3(row_blocks * K), dim3(GETS_THREADS), 0, s, string_buf, string_bytes, value, tag, n, row_blocks, g, value_out, code_out, valid_out,
                     counts);
  hipLaunchKernelGGL(k_cast_strings_exact, dim3(exact_blocks * K), dim3(GETS_EXACT_THREADS), 0, s, string_buf, value, n, exact_blocks, value_out, code_out, valid_out, counts);
  return hipSuccess;
}

} // namespace sjgpu
