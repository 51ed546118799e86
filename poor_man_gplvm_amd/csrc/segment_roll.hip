// Per-neuron circular spike shuffles within events, gfx950: the prepared spikes (the int8
// operand yq, the gammaln constant gconst, and the f32 copy y off the integer path) of R
// shuffled copies of the compact event rows, made on the device from one upload.
//
// The reference rolls every neuron's spike train circularly and independently within the
// epoch and decodes again (reactivation_analysis.py,
// circular_shuffle_spikes_within_epoch_and_decode -> circular_shuffle_column_independently).
// Unlike the time-bin and column-cycle shuffles of segment_shuffle.hip this needs a new
// emission per shuffle; this kernel writes exactly what that emission reads and nothing else
// (no yext, no bf16 transpose, no flags: a roll within an event keeps each neuron's multiset
// of counts, so the int8 / integer eligibility of the source holds for every copy).
//
// For shuffle r, segment s with clamped rows [a, b), len = b - a, row t in [a, b), neuron n:
//   k   = shift[r, s, n] mod len in [0, len)      (64-bit: INT32_MIN is safe)
//   src = a + ((t - a - k) mod len)               (np.roll: out[t] = in[t - k])
//   y_out[r T + t, n] = y[src, n],  yq_out[r T + t, n] = yq[src, n] (columns N .. Kp-1 zero),
//   gconst_out[r T + t] = sum_n ma[n] lgamma(y[src_n, n] + 1).
//
// MI355X design:
//   * a 256-thread workgroup per (segment, shuffle) pair p = s R + r, persistent over the pairs
//     (grid-stride): the R copies of an event are neighbours in the launch and find its source
//     rows in L2;
//   * the lgamma table of k_spikes_prepare (prep.hip) is written once per call by a one-wave
//     kernel into a module array and copied to LDS once per workgroup.  The inlined f64 lgamma
//     costs ~200 VGPRs (2 waves per SIMD), too few waves for a latency-bound gather, so only
//     the instantiation that reads f32 y (values beyond the table take lgamma) carries it;
//     on the int8-only path every value is a count 0 .. 127 by construction (the source's
//     flags were 0) and the table is all it needs -- a negative byte, which that path cannot
//     hold, adds nothing;
//   * the pair's N reduced shifts are staged in LDS once (one 64-bit modulo per neuron per
//     pair, not per row); N > kRollLdsN or an event of 2^31 rows or more reduces at each use;
//   * the four waves stride the event's rows.  With N % 4 == 0 a lane owns 4 consecutive
//     neurons: four byte / dword gathers across the event's rows, one char4 and one float4
//     store per row, as k_spikes_prepare; otherwise the scalar form;
//   * gconst keeps k_spikes_prepare's order (lane l adds neurons l, l + 64, ..., then
//     wave_sum_f64) and its table, so it is bit for bit what pmg_spikes_prepare writes for the
//     host-rolled rows; with y == NULL the sum is formed from the int8 values (the same
//     values under a 0/1 mask);
//   * every source row is a + rel with rel in [0, len), every shift index has r < R, s < S,
//     n < N, every destination row is r T + t < R T: no address leaves the arrays whatever
//     seg_off and shift hold.  Rows that no clamped segment owns are not written.
//   * no atomics, no workspace, plain vector stores only.
#include "pmg_common.h"

namespace pmg {

constexpr int kRollLgfN = 128;     // lgamma(k + 1), k = 0 .. 127, as k_spikes_prepare
constexpr int kRollLdsN = 8192;    // neurons whose reduced shifts are staged in LDS (32 KB)

__device__ __forceinline__ int64_t roll_reduce(int32_t shift, int64_t len) {
  const int64_t k = (int64_t)shift % len;
  return k < 0 ? k + len : k;
}

__device__ double g_roll_lgf[kRollLgfN];

__global__ void __launch_bounds__(kRollLgfN) k_roll_lgamma_table() {
  g_roll_lgf[threadIdx.x] = lgamma((double)threadIdx.x + 1.0);
}

template <bool VEC, bool FROM_Y>
__global__ void __launch_bounds__(256) k_segment_roll(
    const float* __restrict__ y, const int8_t* __restrict__ yq, const float* __restrict__ ma, int64_t T,
    int N, int Kp, const int64_t* __restrict__ seg_off, int S, const int32_t* __restrict__ shift, int R,
    float* __restrict__ y_out, int8_t* __restrict__ yq_out, double* __restrict__ gconst_out, int lds_n) {
  __shared__ double lgf[kRollLgfN];
  extern __shared__ int32_t sk[];   // lds_n reduced shifts of the current pair
  if (threadIdx.x < kRollLgfN) lgf[threadIdx.x] = g_roll_lgf[threadIdx.x];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t pairs = (int64_t)S * R;
  for (int64_t p = blockIdx.x; p < pairs; p += gridDim.x) {
    const int s = (int)(p / R);
    const int r = (int)(p - (int64_t)s * R);
    int64_t a = seg_off[s], b = seg_off[s + 1];   // clamped as seg_rows (segment_table.h)
    a = a < 0 ? 0 : (a > T ? T : a);
    b = b < a ? a : (b > T ? T : b);
    const int64_t len = b - a;
    if (len == 0) continue;   // workgroup-uniform
    const int32_t* sh = shift + ((int64_t)r * S + s) * N;
    const bool staged = lds_n >= N && len <= 0x7fffffffLL;
    __syncthreads();   // the previous pair's rows are done with sk (first pass: lgf is written)
    if (staged)
      for (int n = threadIdx.x; n < N; n += blockDim.x) sk[n] = (int32_t)roll_reduce(sh[n], len);
    __syncthreads();
    // source row of neuron n at row a + rel0
    auto src_row = [&](int n, int64_t rel0) -> int64_t {
      const int64_t k = staged ? (int64_t)sk[n] : roll_reduce(sh[n], len);
      int64_t rel = rel0 - k;
      rel += rel < 0 ? len : 0;
      return a + rel;
    };
    // k_spikes_prepare's spike_elem without the flags
    auto gsum = [&](int n, int64_t src, double& g) {
      const float m = ma ? ma[n] : 1.f;
      if constexpr (FROM_Y) {
        const float v = y[src * N + n];
        const bool small_int = v >= 0.f && v <= 127.f && v == rintf(v);
        if (m != 0.f) g += (double)m * (small_int ? lgf[(int)v] : lgamma((double)v + 1.0));
      } else {
        const int v = yq[src * Kp + n];
        if (m != 0.f && v >= 0) g += (double)m * lgf[v];
      }
    };
    for (int64_t t = a + wv; t < b; t += (blockDim.x >> 6)) {
      const int64_t rel0 = t - a;
      const int64_t o = (int64_t)r * T + t;
      double g = 0.0;
      if constexpr (VEC) {
        const int n4 = N >> 2;
        for (int i = lane; i < (Kp >> 2); i += 64) {
          if (i < n4) {
            const int n = 4 * i;
            const int64_t s0 = src_row(n, rel0), s1 = src_row(n + 1, rel0), s2 = src_row(n + 2, rel0),
                          s3 = src_row(n + 3, rel0);
            if (yq_out) {
              char4 q;
              q.x = yq[s0 * Kp + n];
              q.y = yq[s1 * Kp + n + 1];
              q.z = yq[s2 * Kp + n + 2];
              q.w = yq[s3 * Kp + n + 3];
              *reinterpret_cast<char4*>(yq_out + o * Kp + n) = q;
            }
            if (y_out) {
              float4 v;
              v.x = y[s0 * N + n];
              v.y = y[s1 * N + n + 1];
              v.z = y[s2 * N + n + 2];
              v.w = y[s3 * N + n + 3];
              *reinterpret_cast<float4*>(y_out + o * N + n) = v;
            }
          } else if (yq_out) {
            *reinterpret_cast<char4*>(yq_out + o * Kp + 4 * i) = make_char4(0, 0, 0, 0);
          }
        }
        // gammaln sum in the scalar order (the values are re-read from L1 / L2)
        if (gconst_out)
          for (int n = lane; n < N; n += 64) gsum(n, src_row(n, rel0), g);
      } else {
        for (int n = lane; n < Kp; n += 64) {
          if (n < N) {
            const int64_t src = src_row(n, rel0);
            if (yq_out) yq_out[o * Kp + n] = yq[src * Kp + n];
            if (y_out) y_out[o * N + n] = y[src * N + n];
            if (gconst_out) gsum(n, src, g);
          } else if (yq_out) {
            yq_out[o * Kp + n] = 0;
          }
        }
      }
      if (gconst_out) {   // wave-uniform: every lane takes part in the sum
        g = wave_sum_f64(g);
        if (lane == 0) gconst_out[o] = g;
      }
    }
  }
}

}  // namespace pmg

using namespace pmg;

extern "C" {

int pmg_segment_roll_prepare(const float* y, const int8_t* yq, const float* ma_neuron_1d, int64_t T, int32_t N,
                             int32_t Kp, const int64_t* seg_off, int32_t S, const int32_t* shift, int32_t R,
                             float* y_out, int8_t* yq_out, double* gconst_out, void* stream) {
  PMG_REQUIRE(T > 0 && N > 0, "pmg_segment_roll_prepare: T=%lld N=%d", (long long)T, N);
  PMG_REQUIRE(Kp >= N && Kp % 32 == 0, "pmg_segment_roll_prepare: Kp=%d must be >= N and a multiple of 32", Kp);
  PMG_REQUIRE(S >= 0, "pmg_segment_roll_prepare: S=%d segments (>= 0)", S);
  PMG_REQUIRE(R >= 1, "pmg_segment_roll_prepare: R=%d shuffles (>= 1)", R);
  PMG_REQUIRE((int64_t)S * R <= 0x7fffffffLL, "pmg_segment_roll_prepare: S=%d x R=%d pairs exceed the grid", S, R);
  PMG_REQUIRE(T <= (INT64_MAX >> 3) / R / Kp,
              "pmg_segment_roll_prepare: R=%d x T=%lld rows exceed the int64 byte offsets", R, (long long)T);
  PMG_REQUIRE(y_out || yq_out || gconst_out, "pmg_segment_roll_prepare: every output is null");
  PMG_REQUIRE(!y_out || y, "pmg_segment_roll_prepare: y_out needs y");
  PMG_REQUIRE(!yq_out || yq, "pmg_segment_roll_prepare: yq_out needs yq");
  PMG_REQUIRE(!gconst_out || y || yq, "pmg_segment_roll_prepare: gconst_out needs y or yq");
  PMG_REQUIRE(seg_off, "pmg_segment_roll_prepare: seg_off is null");
  PMG_REQUIRE(shift, "pmg_segment_roll_prepare: shift is null");
  PMG_REQUIRE((!y_out || y_out != y) && (!yq_out || yq_out != yq),
              "pmg_segment_roll_prepare: an output aliases its input");
  hipStream_t st = as_stream(stream);
  const int64_t RT = (int64_t)R * T;
  if (yq_out && round_up(RT, 64) > RT)   // the int8 operand's padding rows
    PMG_HIP(hipMemsetAsync(yq_out + RT * Kp, 0, (size_t)((round_up(RT, 64) - RT) * Kp), st));
  if (S == 0) return PMG_OK;
  const int64_t pairs = (int64_t)S * R;
  const unsigned blocks = (unsigned)(pairs < 4096 ? pairs : 4096);   // persistent over the pairs
  const int lds_n = N <= kRollLdsN ? N : 0;
  const size_t lds = (size_t)lds_n * sizeof(int32_t);
  // the 4-neuron form stores 16 bytes of y_out and 4 of yq_out at a time
  const bool vec = (N & 3) == 0 && ((uintptr_t)y_out & 15) == 0 && ((uintptr_t)yq_out & 3) == 0;
  if (gconst_out) {
    hipLaunchKernelGGL(k_roll_lgamma_table, dim3(1), dim3(kRollLgfN), 0, st);
    PMG_LAUNCH_CHECK();
  }
  auto kf = vec ? (y ? k_segment_roll<true, true> : k_segment_roll<true, false>)
                : (y ? k_segment_roll<false, true> : k_segment_roll<false, false>);
  hipLaunchKernelGGL(kf, dim3(blocks), dim3(256), lds, st, y, yq, ma_neuron_1d, T, N, Kp, seg_off, S, shift, R,
                     y_out, yq_out, gconst_out, lds_n);
  PMG_LAUNCH_CHECK();
  return PMG_OK;
}

}  // extern "C"
