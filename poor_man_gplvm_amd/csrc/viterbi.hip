// Most likely (dynamics, latent) path of the jump GPLVM: a max-plus forward scan with
// compact back-pointers, a streaming back-trace and an f64 path score, gfx950.
//
// The recurrence is filter_one_step (decoder.py:151-172) with each logsumexp replaced
// by a max (the reference has no Viterbi of its own), over the device transition of
// pmg_transition (banded K0, exactly -inf beyond the band; K1 = 1/L):
//   a[d'][i] = max_d (delta_[d][i] + logA[d,d'])
//   v0[j]    = max_{|i-j|<=band} (a[0][i] + log g[|i-j|] + log invz[i])
//   v1       = max_i a[1][i] - log L                      (one scalar and arg-max per step)
//   delta_'[d'][j] = v_d'[j] + s*delta[t,j] + phi[t,j/32]
//
// MI355X design (the per-chain device code is in viterbi_kernels.h, shared with the
// ragged kernel set of segment_viterbi.hip):
//   * one wave per sequence, the filters' lane layout (lane l owns latents lJ .. lJ+J-1,
//     Lpad = 64 J); the band maximum takes its halo from the neighbouring lanes through
//     wave_shr:1 / wave_shl:1 DPP moves (the lanes past either end read -inf), as
//     band_conv does for sums; no LDS on the step;
//   * the f32 scores are re-centred every step by the largest a[d'][i] (one monotone
//     subtraction, so no arg-max moves): they stay within the emission's range however
//     long the sequence;
//   * emission rows are prefetched PF steps ahead through the buffer-load row ring of
//     fwd_stream;
//   * back-pointers: one byte per (t, j), bits 0..6 = i - j + band of v0[j]'s maximiser,
//     bit 7 = the previous dynamics chosen by a[0][j] (indexed by the PREDECESSOR j, so
//     the back-trace reads byte [t][j] then bit 7 of byte [t][i], both in row t); one
//     int32 per t for the jump state, i | d << 16;
//   * back-trace: one wave per sequence streams whole back-pointer rows, a piece of rows
//     at a time (coalesced 16-byte loads, the next piece in flight in registers while the
//     current one is walked in LDS); no dependent global load per step;
//   * score: a T-parallel gather of the path's per-step increments in f64 (ll as
//     rblk + delta, the transition logs from the f32 device values), reduced in a fixed
//     order.  Nothing of the f32 scan enters it.
#include "viterbi_kernels.h"

namespace pmg {

template <int J, int WP>
__global__ void __launch_bounds__(64) k_viterbi_fwd(VitParams p) {
  const VitSeq ch = {(int)blockIdx.y};
  if constexpr (J % 4 == 0) {
    if ((p.L & 3) == 0) {
      vit_forward<J, WP, 1>(p, ch);
      return;
    }
  }
  vit_forward<J, WP, 0>(p, ch);
}

__global__ void __launch_bounds__(64) k_viterbi_trace(VitParams p) {
  const VitSeq ch = {(int)blockIdx.x};
  vit_trace(p, ch);
}

// per-step increments of log p(x, y) along the path, f64
__global__ void __launch_bounds__(256) k_viterbi_inc(VitParams p) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.T * p.R) return;
  vit_increment(p, idx, idx % p.T == 0);
}

// log_joint[r] = sum_t inc[r][t]: thread i adds steps i, i + 256, ... in order, then a
// fixed tree over the 256 partial sums (the same order whatever R is)
__global__ void __launch_bounds__(256) k_viterbi_sum(VitParams p) {
  __shared__ double part[256];
  const int r = blockIdx.x;
  const double v = vit_sum(p.inc + (int64_t)r * p.T, p.T, part);
  if (threadIdx.x == 0) p.log_joint[r] = v;
}

// ---------------------------------------------------------------------------
// host dispatch
// ---------------------------------------------------------------------------
typedef void (*vit_kernel_t)(VitParams);
static vit_kernel_t vit_kernel(int J, int WP) {
#define PMG_VIT_CASE(JJ, WW) \
  if (J == JJ && WP == WW) return k_viterbi_fwd<JJ, WW>;
  PMG_VIT_ALL(PMG_VIT_CASE)
#undef PMG_VIT_CASE
  return nullptr;
}

struct VitWork {
  uint8_t* bp;
  int32_t* jp;
  int32_t* last;
  double* inc;
};

static VitWork carve_vit(void* ws, int64_t T, int Lpad, int R, size_t* total = nullptr) {
  Carver c(ws);
  VitWork w;
  w.bp = c.take<uint8_t>((size_t)R * T * Lpad);
  w.jp = c.take<int32_t>((size_t)R * T);
  w.last = c.take<int32_t>((size_t)R * 2);
  w.inc = c.take<double>((size_t)R * T);
  if (total) *total = c.off + 256;
  return w;
}

}  // namespace pmg

using namespace pmg;

extern "C" {

size_t pmg_viterbi_workspace_size(int64_t T, int32_t L, int32_t R) {
  const int J = vit_J(L);
  if (J < 0 || T <= 0 || R < 1 || R > 65535) return 0;
  size_t total = 0;
  carve_vit(nullptr, T, 64 * J, R, &total);
  return total;
}

int pmg_viterbi_decode(const float* delta, const float* phi, const double* rblk, int64_t T, int32_t R,
                       const pmg_transition* tr, const double* log_pi0, double likelihood_scale,
                       int32_t* path_d, int32_t* path_l, double* log_joint, void* workspace,
                       size_t workspace_bytes, void* stream) {
  PMG_REQUIRE(T > 0, "pmg_viterbi_decode: T=%lld must be > 0", (long long)T);
  PMG_REQUIRE(R >= 1 && R <= 65535, "pmg_viterbi_decode: R=%d sequences (1 .. 65535)", R);
  PMG_REQUIRE(delta, "pmg_viterbi_decode: delta is null");
  PMG_REQUIRE(phi, "pmg_viterbi_decode: phi is null");
  PMG_REQUIRE(rblk, "pmg_viterbi_decode: rblk is null");
  PMG_REQUIRE(tr, "pmg_viterbi_decode: tr is null");
  PMG_REQUIRE(tr->L > 0 && tr->invz, "pmg_viterbi_decode: tr: bad transition (L=%d, invz %s)", tr->L,
              tr->invz ? "set" : "null");
  PMG_REQUIRE(tr->band >= 0 && tr->band <= kMaxBand && tr->band < tr->L,
              "pmg_viterbi_decode: tr: continuous-kernel band %d outside [0, min(%d, L-1)] (dense kernels: unsupported)",
              tr->band, kMaxBand);
  PMG_REQUIRE(log_pi0, "pmg_viterbi_decode: log_pi0 is null");
  PMG_REQUIRE(likelihood_scale == likelihood_scale, "pmg_viterbi_decode: likelihood_scale is NaN");
  PMG_REQUIRE(path_d, "pmg_viterbi_decode: path_d is null");
  PMG_REQUIRE(path_l, "pmg_viterbi_decode: path_l is null");
  PMG_REQUIRE(log_joint, "pmg_viterbi_decode: log_joint is null");
  PMG_REQUIRE(workspace, "pmg_viterbi_decode: workspace is null");
  const int J = vit_J(tr->L);
  if (J < 0) {
    set_error("pmg_viterbi_decode: L=%d > 1024 unsupported", tr->L);
    return PMG_EUNSUPPORTED;
  }
  const size_t need = pmg_viterbi_workspace_size(T, tr->L, R);
  PMG_REQUIRE(workspace_bytes >= need, "pmg_viterbi_decode: workspace_bytes %zu < %zu", workspace_bytes, need);
  const int64_t cells = T * (int64_t)R;
  PMG_REQUIRE((cells + 255) / 256 <= 0x7fffffffll, "pmg_viterbi_decode: T * R = %lld too large", (long long)cells);

  VitParams p;
  vit_fill_params(p, tr, J, likelihood_scale);
  p.delta = delta;
  p.phi = phi;
  p.rblk = rblk;
  p.log_pi0 = log_pi0;
  p.T = T;
  p.R = R;
  const VitWork w = carve_vit(workspace, T, p.Lpad, R);
  p.bp = w.bp;
  p.jp = w.jp;
  p.last = w.last;
  p.inc = w.inc;
  p.path_d = path_d;
  p.path_l = path_l;
  p.log_joint = log_joint;

  const vit_kernel_t kf = vit_kernel(J, vit_WP(tr->band));
  PMG_REQUIRE(kf, "pmg_viterbi_decode: no kernel for J=%d band=%d", J, tr->band);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(kf, dim3(1, R), dim3(64), 0, st, p);
  PMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_viterbi_trace, dim3(R), dim3(64), 0, st, p);
  PMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_viterbi_inc, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, p);
  PMG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_viterbi_sum, dim3(R), dim3(256), 0, st, p);
  PMG_LAUNCH_CHECK();
  return PMG_OK;
}

}  // extern "C"
