// simdjson_amd/csrc/sj_cell_kinds.h -- the census slot of a cell's tag byte (include/sjgpu_cast.h: the sixteen counters of sjgpu_cell_kinds_device), stated ONCE for
// the kernels that count by it: k_cell_kinds (sjgpu_cast.hip, one census per row) and k_cell_kinds_by_code (sjgpu_dict.hip, one census per dictionary code).
#ifndef SJ_CELL_KINDS_H
#define SJ_CELL_KINDS_H

#include "sjgpu_device.h"

namespace sjgpu {
namespace {

constexpr u32 KIND_SLOTS = 16, KIND_NEGATIVE = 9, KIND_OTHER = 14, KIND_NONE = 15;

// the census slot of a tag byte (include/sjgpu_cast.h); slot 9 is not a tag's
__device__ __forceinline__ u32 kind_slot(u32 t) {
  switch (t) {
    case '{': return 0;
    case '[': return 1;
    case '"': return 2;
    case 'l': return 3;
    case 'u': return 4;
    case 'd': return 5;
    case 't': return 6;
    case 'f': return 7;
    case 'n': return 8;
    case 17: return 10;
    case 19: return 11;
    case 20: return 12;
    case 22: return 13;
    default: return KIND_OTHER;
  }
}

} // namespace
} // namespace sjgpu
#endif
