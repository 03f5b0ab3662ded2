// simdjson_amd/csrc/sjgpu_dict.hip -- dictionary-encode a row of string cells (sjgpu_dictionary_encode_device) and the census of a value row per dictionary code
// (sjgpu_cell_kinds_by_code_device).  Contract: include/sjgpu_dict.h.
//
// The encode reads one row of n cells and the string buffer, no tape.  Workspace (dict_workspace_bytes): [ctrl, 256 bytes][table: S u32][count: S u32][slot_of: n u32]
// [rank: n + 2 ints][the scan's block sums], S the smallest power of two >= 2 n.
//   k_dict_insert   one lane per row.  A string cell hashes its bytes (64 bits, the length mixed in) and probes the open-addressed table linearly: an empty slot
//                   (0xFFFFFFFF) is claimed with a compare-and-swap of the row, an occupied one is compared with the lane's own string -- the same cell word, or
//                   the same length and the same bytes -- and is the string's slot when equal.  The probe is bounded by S steps and never waits: at load <= 0.5 it
//                   cannot run out, and if it does it raises rank[n + 1], which the C entry returns as SJGPU_E_INTERNAL.  The lanes of a wave that read "empty"
//                   at one slot elect one to try the compare-and-swap and share its outcome.  A slot is read with a relaxed load that
//                   may be stale (another XCD's L2): stale is either "empty", and then the compare-and-swap answers with the truth, or an earlier occupant, and
//                   every occupant a slot ever has holds the same bytes (a slot never empties again and only atomicMin replaces its row).
//                   BEHIND the divergent loop, with the whole wave in every ballot, the lanes that found the same slot elect their lowest -- rows are consecutive,
//                   so it holds the smallest row -- and only that lane does one atomicAdd of the group's popcount into count[slot], and one atomicMin of its row
//                   into the slot unless the row it saw there is already no larger: a wave of one distinct string is one or two atomics, not 128.
//   k_dict_heads    row r is a HEAD when table[slot_of[r]] == r: the first occurrence of its string.  rank[r] = its flag, rank[n] = 0, ctrl = n + 1.
//   enqueue_scan    the exclusive scan of the flags in place (sjgpu_finish.hip): rank[r] of a head is its dictionary index, rank[n] the number of distinct strings
//                   (at most n <= 2^30: the scan's 32-bit words hold it, no 64-bit total is needed).
//   k_dict_codes    codes[r] = rank[table[slot_of[r]]], -1 for a null.  They do not depend on the capacity and are complete before the total is read back.
//   k_dict_fill     (when the total fits) a head writes entry rank[r]: its row, its cell word, '"' and count[slot_of[r]].
// First occurrence, counts and codes are functions of the row alone: which lane claimed a slot, and in what order the probes met, shows nowhere.
// One lane hashes and compares its own string: a string of a megabyte is ONE lane's work (include/sjgpu_dict.h, "Cost, not hidden").
#include "sjgpu_device.h"
#include "sjgpu_dict.h"
#include "sj_cell_kinds.h"

// the hash's width, cut by the CPU tier alone (tests/test_dict_emu.py builds this unit a second time with 3 bits: every string then meets equal hashes with unequal
// bytes and long probe chains, and the outputs must not change)
#ifndef SJGPU_DICT_HASH_BITS
#define SJGPU_DICT_HASH_BITS 64
#endif

namespace sjgpu {
namespace {

constexpr u32 DICT_THREADS = 256;
constexpr u32 DICT_EMPTY = 0xFFFFFFFFu, DICT_NO_SLOT = 0xFFFFFFFFu; // (S <= 2^31: no slot has this index, no row this number)
constexpr u64 DICT_MUL = 0x9E3779B97F4A7C15ull, LOW32 = 0xFFFFFFFFull;
static_assert(SJGPU_DICT_HASH_BITS >= 1 && SJGPU_DICT_HASH_BITS <= 64, "the hash is 1 .. 64 bits wide");

// compare-and-swap of one table slot -> what the slot held.  (tests/host/emu/hip/hip_runtime.h has no atomicCAS)
__device__ __forceinline__ u32 slot_cas(u32 *p, u32 expected, u32 desired) {
#if defined(SJ_EMU)
  __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
  return expected;
#else
  return atomicCAS(p, expected, desired);
#endif
}

__device__ __forceinline__ u64 load_u64_unaligned(const u8 *p) {
  u64 w;
  __builtin_memcpy(&w, p, sizeof w);
  return w;
}

__device__ __forceinline__ u64 mix64(u64 h) {
  h ^= h >> 32;
  h *= DICT_MUL;
  h ^= h >> 29;
  return h;
}

// the hash of s[0 .. len): whole 8-byte words, then the tail's bytes as one word; nothing outside the string is read
__device__ __forceinline__ u64 hash_string(const u8 *s, u32 len) {
  u64 h = mix64(u64(len) + DICT_MUL);
  u32 i = 0;
  for (; i + 8u <= len; i += 8u) { h = mix64(h ^ load_u64_unaligned(s + i)); }
  if (i < len) {
    u64 w = 0;
    for (u32 k = 0; i + k < len; k++) { w |= u64(s[i + k]) << (8u * k); }
    h = mix64(h ^ w);
  }
#if SJGPU_DICT_HASH_BITS < 64
  h &= (1ull << SJGPU_DICT_HASH_BITS) - 1ull;
#endif
  return h;
}

__device__ __forceinline__ bool same_bytes(const u8 *a, const u8 *b, u32 len) {
  u32 i = 0;
  for (; i + 8u <= len; i += 8u) {
    if (load_u64_unaligned(a + i) != load_u64_unaligned(b + i)) { return false; }
  }
  for (; i < len; i++) {
    if (a[i] != b[i]) { return false; }
  }
  return true;
}

// a string cell inside the buffer (the rule of k_gather_lengths)
__device__ __forceinline__ bool is_string_cell(u32 t, u64 w, u64 string_bytes) { return t == '"' && (w & LOW32) + (w >> 32) <= string_bytes; }

// one lane's probe: where it looks, what it looks for, and what came of it
struct dict_probe {
  u64 w;          // the lane's cell word
  const u8 *mine; // its string
  u32 len, at;    // its length; the slot to look at next
  u32 slot, known; // the string's slot once found, and the row the lane saw in it (its own when it claimed it)
  u64 steps;
  bool active;
};

// the lane has read `held` in slot P.at (DICT_EMPTY: it has just claimed the slot for `row`): its string's slot, or on to the next one
__device__ __forceinline__ void dict_settle(dict_probe &P, u32 held, u32 row, const u64 *__restrict__ value, const u8 *__restrict__ sbuf, u32 mask, int *failed) {
  bool found = held == DICT_EMPTY;
  if (found) {
    held = row;
  } else {
    const u64 other = value[held]; // a row that entered the table is a string cell inside the buffer
    found = other == P.w || (u32(other >> 32) == P.len && same_bytes(P.mine, sbuf + (other & LOW32), P.len));
  }
  if (found) {
    P.slot = P.at;
    P.known = held;
    P.active = false;
    return;
  }
  P.at = (P.at + 1u) & mask;
  if (++P.steps > mask) { // cannot happen at load <= 0.5: reported, not looped on
    atomicOr(failed, 1);
    P.active = false;
  }
}

// rank[n + 1]: the flag of a probe that ran out (zeroed by the launcher).
// The first DICT_WAVE_ROUNDS steps of the probe are taken by the wave together: the lanes that read "empty" at the same slot elect ONE of them to try the
// compare-and-swap and take its outcome from it.  A column of one value, read by half a million resident lanes before the first claim has landed, would otherwise
// queue one returning atomic per CELL on one word (measured: 1.0 ms for 344 727 rows of one string, against 0.17 ms for as many distinct ones).  Whoever is still
// looking after that goes on alone, lane by lane: those are collisions, not herds.
constexpr u32 DICT_WAVE_ROUNDS = 2;
__global__ __launch_bounds__(DICT_THREADS) void k_dict_insert(const u64 *__restrict__ value, const u8 *__restrict__ tag, u32 n, const u8 *__restrict__ sbuf, u64 string_bytes,
                                                              u32 mask, u32 *table, u32 *count, u32 *__restrict__ slot_of, int *failed) {
  const u64 i64 = u64(blockIdx.x) * DICT_THREADS + threadIdx.x;
  const u32 row = u32(i64), lane = lane_id();
  const bool in = i64 < n;
  dict_probe P = {0, sbuf, 0, 0, DICT_NO_SLOT, DICT_EMPTY, 0, false};
  if (in) { P.w = value[row]; }
  P.active = in && is_string_cell(tag[row], P.w, string_bytes);
  if (P.active) {
    P.len = u32(P.w >> 32);
    P.mine = sbuf + (P.w & LOW32);
    const u64 h = hash_string(P.mine, P.len);
    P.at = u32(h ^ (h >> 32)) & mask;
  }
  for (u32 round = 0; round < DICT_WAVE_ROUNDS && __ballot(P.active); round++) { // uniform over the wave
    u32 held = DICT_EMPTY;
    if (P.active) { held = __hip_atomic_load(table + P.at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    const bool wants = P.active && held == DICT_EMPTY;
    u32 elector = lane;
    u64 todo = __ballot(wants);
    while (todo) { // once per slot that some lane read empty
      const u32 leader = ctz64(todo);
      const u32 its = readlane_dyn(P.at, leader);
      const bool mine_too = wants && P.at == its;
      if (mine_too) { elector = leader; }
      todo &= ~__ballot(mine_too);
    }
    if (wants && elector == lane) { held = slot_cas(table + P.at, DICT_EMPTY, row); } // DICT_EMPTY back: claimed
    const u32 electors_held = u32(__shfl(int(held), int(elector))), electors_row = u32(__shfl(int(row), int(elector)));
    if (wants && elector != lane) { held = electors_held == DICT_EMPTY ? electors_row : electors_held; } // what the slot holds now, or held a moment ago
    if (P.active) { dict_settle(P, held, row, value, sbuf, mask, failed); }
  }
  while (P.active) { // S steps at the most, the wave's rounds included: no lane waits for another
    u32 held = __hip_atomic_load(table + P.at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (held == DICT_EMPTY) { held = slot_cas(table + P.at, DICT_EMPTY, row); }
    dict_settle(P, held, row, value, sbuf, mask, failed);
  }
  const u32 slot = P.slot, known = P.known;
  if (in) { slot_of[row] = slot; }
  // the lanes of one slot elect their lowest, which holds the smallest row: one atomicAdd of the group's size, and an atomicMin only where the slot may still hold
  // a larger row (what a lane saw there is never below what is there now: a slot's row only falls)
  u64 todo = __ballot(slot != DICT_NO_SLOT);
  while (todo) { // uniform over the wave
    const u32 leader = ctz64(todo);
    const u32 its = readlane_dyn(slot, leader);
    const u64 group = __ballot(slot == its);
    if (lane == leader) {
      if (row < known) { atomicMin(table + its, row); }
      atomicAdd(count + its, u32(__popcll(group)));
    }
    todo &= ~group;
  }
}

__device__ __forceinline__ bool is_head(const u32 *table, u32 slot, u32 row) { return slot != DICT_NO_SLOT && table[slot] == row; }

// rank[r] = 1 for a head, rank[n] = 0; ctrl[0] = n + 1, the length of the scan
__global__ __launch_bounds__(DICT_THREADS) void k_dict_heads(const u32 *__restrict__ table, const u32 *__restrict__ slot_of, u32 n, int *__restrict__ rank, u32 *__restrict__ ctrl) {
  const u64 r = u64(blockIdx.x) * DICT_THREADS + threadIdx.x;
  if (r == 0) { ctrl[0] = n + 1u; }
  if (r > n) { return; }
  rank[r] = r < n && is_head(table, slot_of[r], u32(r)) ? 1 : 0;
}

__global__ __launch_bounds__(DICT_THREADS) void k_dict_codes(const u32 *__restrict__ table, const u32 *__restrict__ slot_of, const int *__restrict__ rank, u32 n,
                                                             int *__restrict__ codes) {
  const u64 r = u64(blockIdx.x) * DICT_THREADS + threadIdx.x;
  if (r >= n) { return; }
  const u32 slot = slot_of[r];
  codes[r] = slot == DICT_NO_SLOT ? -1 : rank[table[slot]];
}

__global__ __launch_bounds__(DICT_THREADS) void k_dict_fill(const u64 *__restrict__ value, const u32 *__restrict__ table, const u32 *__restrict__ count,
                                                            const u32 *__restrict__ slot_of, const int *__restrict__ rank, u32 n, u64 *__restrict__ dict_value,
                                                            u8 *__restrict__ dict_tag, u32 *__restrict__ dict_first, u32 *__restrict__ dict_count) {
  const u64 r = u64(blockIdx.x) * DICT_THREADS + threadIdx.x;
  if (r >= n) { return; }
  const u32 slot = slot_of[r];
  if (!is_head(table, slot, u32(r))) { return; }
  const u32 j = u32(rank[r]);
  dict_value[j] = value[r];
  dict_tag[j] = '"';
  dict_first[j] = u32(r);
  dict_count[j] = count[slot];
}

// ---- the census by code ----------------------------------------------------------------------------------------------------------------------------------
constexpr u32 BY_CODE_LDS_GROUPS = 512;       // 512 x 16 counters = 32 KiB of LDS per workgroup
constexpr u32 BY_CODE_MAX_WORKGROUPS = 1024;  // each flushes its non-zero counters once: more workgroups are more atomics on the same words

// (slot, negative) of one cell; KIND_NONE for a cell that is counted nowhere
__device__ __forceinline__ u32 cell_slot(const u8 *s_slot, u32 t, u64 w, bool *negative) {
  *negative = t == 'l' && w >= 0x8000000000000000ull;
  return s_slot[t];
}

// groups <= BY_CODE_LDS_GROUPS: the histogram of the workgroup's cells in LDS, one global atomicAdd per non-zero counter and workgroup
__global__ __launch_bounds__(DICT_THREADS) void k_cell_kinds_by_code_lds(const int *__restrict__ codes, const u64 *__restrict__ value, const u8 *__restrict__ tag, u32 n,
                                                                         u32 groups, u32 *__restrict__ kinds) {
  __shared__ u32 s_hist[BY_CODE_LDS_GROUPS * KIND_SLOTS];
  __shared__ u8 s_slot[256]; // kind_slot of every byte (256 lanes, 256 bytes), as in k_cell_kinds
  const u32 counters = groups * KIND_SLOTS;
  s_slot[threadIdx.x] = u8(kind_slot(threadIdx.x));
  for (u32 c = threadIdx.x; c < counters; c += DICT_THREADS) { s_hist[c] = 0; }
  lds_writes_done();
  __syncthreads();
  const u64 stride = u64(gridDim.x) * DICT_THREADS;
  for (u64 i = u64(blockIdx.x) * DICT_THREADS + threadIdx.x; i < n; i += stride) {
    const u32 code = u32(codes[i]); // (-1 and every other negative code: beyond any groups)
    const u32 t = tag[i];
    const u64 w = value[i];
    if (code < groups) {
      bool negative;
      const u32 slot = cell_slot(s_slot, t, w, &negative);
      atomicAdd(&s_hist[code * KIND_SLOTS + slot], 1u);
      if (negative) { atomicAdd(&s_hist[code * KIND_SLOTS + KIND_NEGATIVE], 1u); }
    }
  }
  lds_writes_done();
  __syncthreads();
  for (u32 c = threadIdx.x; c < counters; c += DICT_THREADS) {
    const u32 sum = s_hist[c];
    if (sum) { atomicAdd(&kinds[c], sum); }
  }
}

// more groups than LDS holds: one or two global atomics per counted cell
__global__ __launch_bounds__(DICT_THREADS) void k_cell_kinds_by_code_global(const int *__restrict__ codes, const u64 *__restrict__ value, const u8 *__restrict__ tag, u32 n,
                                                                            u32 groups, u32 *__restrict__ kinds) {
  __shared__ u8 s_slot[256];
  s_slot[threadIdx.x] = u8(kind_slot(threadIdx.x));
  lds_writes_done();
  __syncthreads();
  const u64 stride = u64(gridDim.x) * DICT_THREADS;
  for (u64 i = u64(blockIdx.x) * DICT_THREADS + threadIdx.x; i < n; i += stride) {
    const u32 code = u32(codes[i]);
    const u32 t = tag[i];
    const u64 w = value[i];
    if (code < groups) {
      bool negative;
      const u32 slot = cell_slot(s_slot, t, w, &negative);
      atomicAdd(&kinds[u64(code) * KIND_SLOTS + slot], 1u);
      if (negative) { atomicAdd(&kinds[u64(code) * KIND_SLOTS + KIND_NEGATIVE], 1u); }
    }
  }
}

static inline u32 dict_blocks(u64 n, u32 per) { return u32((n + per - 1) / per); }
static inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

struct dict_workspace {
  u32 *ctrl, *table, *count, *slot_of;
  int *rank, *partial;
  u32 slots;
  size_t bytes;
};

static inline dict_workspace carve_dict_workspace(void *base, u32 n) {
  dict_workspace w;
  u32 S = 2;
  while (S < 2ull * n) { S <<= 1; } // n <= 2^30: S <= 2^31
  w.slots = S;
  uint8_t *p = static_cast<uint8_t *>(base);
  size_t at = 0;
  w.ctrl = reinterpret_cast<u32 *>(p + at);    at += 256;
  w.table = reinterpret_cast<u32 *>(p + at);   at += up256(size_t(S) * sizeof(u32));
  w.count = reinterpret_cast<u32 *>(p + at);   at += up256(size_t(S) * sizeof(u32));
  w.slot_of = reinterpret_cast<u32 *>(p + at); at += up256(size_t(n) * sizeof(u32));
  w.rank = reinterpret_cast<int *>(p + at);    at += up256((size_t(n) + 2) * sizeof(int));
  w.partial = reinterpret_cast<int *>(p + at); at += up256((size_t(dict_blocks(u64(n) + 1, 4096)) + 64) * sizeof(int));
  w.bytes = at;
  return w;
}

} // namespace

size_t dict_workspace_bytes(uint32_t n) { return carve_dict_workspace(nullptr, n).bytes; }

hipError_t launch_dict_encode(const uint64_t *value, const uint8_t *tag, uint32_t n, const uint8_t *string_buf, uint64_t string_bytes, int32_t *codes, void *workspace,
                              hipStream_t s, const dict_result_dev **result) {
  const dict_workspace w = carve_dict_workspace(workspace, n);
  *result = reinterpret_cast<const dict_result_dev *>(w.rank + n);
  hipError_t e = hipMemsetAsync(w.table, 0xFF, size_t(w.slots) * sizeof(u32), s);
  if (e == hipSuccess) { e = hipMemsetAsync(w.count, 0, size_t(w.slots) * sizeof(u32), s); }
  if (e == hipSuccess) { e = hipMemsetAsync(w.rank + n, 0, 2 * sizeof(int), s); }
  if (e != hipSuccess) { return e; }
  const u32 blocks = dict_blocks(n, DICT_THREADS);
  hipLaunchKernelGGL(k_dict_insert, dim3(blocks), dim3(DICT_THREADS), 0, s, value, tag, n, string_buf, string_bytes, w.slots - 1u, w.table, w.count, w.slot_of, w.rank + n + 1);
  hipLaunchKernelGGL(k_dict_heads, dim3(dict_blocks(u64(n) + 1, DICT_THREADS)), dim3(DICT_THREADS), 0, s, w.table, w.slot_of, n, w.rank, w.ctrl);
  enqueue_scan(w.rank, n + 1u, w.ctrl, w.partial, s);
  hipLaunchKernelGGL(k_dict_codes, dim3(blocks), dim3(DICT_THREADS), 0, s, w.table, w.slot_of, w.rank, n, codes);
  return hipSuccess;
}

void launch_dict_fill(const uint64_t *value, uint32_t n, void *workspace, uint64_t *dict_value, uint8_t *dict_tag, uint32_t *dict_first, uint32_t *dict_count, hipStream_t s) {
  const dict_workspace w = carve_dict_workspace(workspace, n);
  hipLaunchKernelGGL(k_dict_fill, dim3(dict_blocks(n, DICT_THREADS)), dim3(DICT_THREADS), 0, s, value, w.table, w.count, w.slot_of, w.rank, n, dict_value, dict_tag, dict_first,
                     dict_count);
}

hipError_t launch_cell_kinds_by_code(const int32_t *codes, const uint64_t *value, const uint8_t *tag, uint32_t n, uint32_t groups, uint32_t *kinds, hipStream_t s) {
  if (groups == 0) { return hipSuccess; }
  const hipError_t e = hipMemsetAsync(kinds, 0, size_t(groups) * KIND_SLOTS * sizeof(u32), s);
  if (e != hipSuccess || n == 0) { return e; }
  const u32 all = dict_blocks(n, DICT_THREADS), blocks = all < BY_CODE_MAX_WORKGROUPS ? all : BY_CODE_MAX_WORKGROUPS;
  if (groups <= BY_CODE_LDS_GROUPS) {
    hipLaunchKernelGGL(k_cell_kinds_by_code_lds, dim3(blocks), dim3(DICT_THREADS), 0, s, codes, value, tag, n, groups, kinds);
  } else {
    hipLaunchKernelGGL(k_cell_kinds_by_code_global, dim3(blocks), dim3(DICT_THREADS), 0, s, codes, value, tag, n, groups, kinds);
  }
  return hipSuccess;
}

} // namespace sjgpu
