// The chain table of the one-wave-per-chain kernel sets (segments.hip, segment_sample.hip,
// viterbi.hip): which rows of the call a workgroup walks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pmg {

struct SegTable {
  const int64_t* seg_off;  // (S + 1) row offsets of a ragged set; null: S chains of `len` rows each
  const int32_t* order;    // (S) chain of each workgroup (ragged set only), or null
  int64_t len;             // rows per chain when seg_off is null
  int S;
};

__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
  const int hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

// chain s of workgroup (group) `grp` and its rows [a, b) of the call's T rows; false:
// nothing to do.  A ragged set's offsets are clamped to 0 <= a <= b <= T (the entry point
// cannot read them); the equal-length rows come from the entry point's own arguments.
__device__ __forceinline__ bool seg_rows(const SegTable& st, int64_t T, int grp, int& s, int64_t& a, int64_t& b) {
  if (!st.seg_off) {   // wave-uniform
    s = grp;
    a = s * st.len;
    b = a + st.len;
    return true;
  }
  s = st.order ? __builtin_amdgcn_readfirstlane(st.order[grp]) : grp;
  if ((unsigned)s >= (unsigned)st.S) return false;
  a = uniform_i64(st.seg_off[s]);
  b = uniform_i64(st.seg_off[s + 1]);
  a = a < 0 ? 0 : (a > T ? T : a);
  b = b < a ? a : (b > T ? T : b);
  return true;
}

}  // namespace pmg
