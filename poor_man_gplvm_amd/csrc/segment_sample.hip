// Joint posterior path samples of many short, independent chains (events: ripple or replay
// candidates, trials), gfx950: the backward-sampling half of forward filtering, backward
// sampling (FFBS) over the filter posteriors alpha that pmg_segment_smoother (or the
// chunk-parallel forward) stored.
//
// The reference has no sampler.  The recursion is the factorisation of smooth_one_step's
// pairwise joint (decoder.py:200-226): p(x_t | x_{t+1}, y) ~ alpha_t[x_t] Trans[x_t, x_{t+1}],
// drawn from t = b-1 down to a, once per (segment, sample).
//
// MI355X design:
//   * the parallel axes are the segments and the samples: one 64-lane wave per (segment,
//     sample); workgroup b takes segment order[b / R] and sample b % R, so the R samples of an
//     event are neighbours in the launch and share its alpha rows in L2;
//   * the lane layout is the scans' (lane l owns latents lJ .. lJ+J-1, Lpad = 64 J); the two
//     alpha rows and the step's uniform are prefetched PF steps ahead in a register ring whose
//     addresses are clamped to the segment's first row, as seg_backward does;
//   * the transition enters through the drawn state alone: the column of K0 at l+ has at most
//     2 band + 1 non-zero taps g[|l - l+|] invz[l], read from a 64-entry LDS table that is zero
//     beyond the band (a per-lane index into the kernel arguments would go through scratch);
//     so J and VEC are the only template parameters;
//   * the draw is the smallest x = d L + l with cdf[x] > u total: the lane's J weights are
//     summed in latent order, the lane sums of each dynamics row go through a 6-step
//     Hillis-Steele wave scan, the d = 1 row adds the d = 0 total; the lane is found by
//     ballot + count-trailing-zeros and walks its J values.  Only states of weight > 0 are
//     candidates at either level, so a masked latent, a latent beyond the band or a zero of A
//     is never returned; where rounding leaves no candidate above the target, the last state
//     of weight > 0 is taken;
//   * no random numbers are made here: the paths are a deterministic function of
//     (alpha, transition, uniforms);
//   * total == 0 or not finite: the wave writes -1 into the rows it has not drawn yet and
//     sets the sticky status word.  No LDS beyond the table, no grid barrier, no atomics.
#include "fb_kernels.h"
#include "segment_table.h"

namespace pmg {

struct SampleParams {
  const float* alpha;      // (T, 2, L)
  const float* invz;       // (L)
  const float* uniforms;   // (R, T)
  SegTable seg;            // the segments' rows (seg_off set), one per group of R workgroups
  int32_t* path_d;         // (R, T)
  int32_t* path_l;         // (R, T)
  int32_t* status;         // (1) sticky
  int64_t T;
  int L, band, R;
  float A00, A01, A10, A11;
  float g[kMaxBand + 1];   // zero beyond the band
};

// ring depth: many waves per SIMD (one per sample), so a shallow ring; a slot is 2 J + 1 floats
template <int J> constexpr int samp_pf() { return J >= 8 ? 2 : 4; }

template <int J>
struct SampRow {
  RowV<J> a0, a1;
  float u;   // the same value in every lane
};

template <int J, int VEC>
__device__ __forceinline__ void samp_row_load(const SampleParams& p, const float* urow, int64_t t, int j0,
                                              SampRow<J>& r) {
  const float* arow = p.alpha + t * 2 * (int64_t)p.L;
  bload_row<J, VEC>(arow, p.L, j0, r.a0);
  bload_row<J, VEC>(arow + p.L, p.L, j0, r.a1);
  r.u = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc_of(urow + t, 4u), 0, 0, 0));
}

// one int32 written by lane 0 only (the other lanes' offsets are out of range)
__device__ __forceinline__ void bstore_i32_lane0(int32_t* base, int64_t t, int32_t v) {
  const __amdgpu_buffer_rsrc_t rs = rsrc_of(base + t, 4u);
  const int off = threadIdx.x == 0 ? 0 : 64;
  __builtin_amdgcn_raw_buffer_store_b32((unsigned)v, rs, off, 0, 0);
}

// inclusive Hillis-Steele scan over the 64 lanes (6 adds deep), two values at once
__device__ __forceinline__ void wave_scan2(int lane, float& a, float& b) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float ua = __shfl_up(a, d, 64);
    const float ub = __shfl_up(b, d, 64);
    if (lane >= d) {
      a += ua;
      b += ub;
    }
  }
}

template <int J, int VEC>
__device__ __forceinline__ void seg_sample(const SampleParams& p, const float* sg) {
  constexpr int PF = samp_pf<J>();
  const int blk = blockIdx.x;
  const int grp = blk / p.R;
  const int r = blk - grp * p.R;
  int s;
  int64_t t_a, t_b;
  __builtin_assume(p.seg.seg_off != nullptr);   // the ragged set only: no equal-length branch here
  if (!seg_rows(p.seg, p.T, grp, s, t_a, t_b) || t_a >= t_b) return;
  PMG_FB_LANE_SETUP
  const float* urow = p.uniforms + (int64_t)r * p.T;
  int32_t* pd = p.path_d + (int64_t)r * p.T;
  int32_t* pl = p.path_l + (int64_t)r * p.T;
  int dn = -1, ln = 0;   // the state drawn at t + 1 (dn < 0: none, t is the segment's last row)
  SampRow<J> ring[PF];
#pragma unroll
  for (int q = 0; q < PF; ++q) samp_row_load<J, VEC>(p, urow, t_b - 1 - q > t_a ? t_b - 1 - q : t_a, j0, ring[q]);

  auto body = [&](int q, int64_t t, bool refill) -> bool {
    float w0[J], w1[J];
    if (dn == 0) {   // wave-uniform
#pragma unroll
      for (int j = 0; j < J; ++j) {
        int k = j0 + j - ln;
        k = k < 0 ? -k : k;
        const float gk = sg[k < 63 ? k : 63];
        w0[j] = ((ring[q].a0[j] * p.A00) * gk) * invz[j];
        w1[j] = ((ring[q].a1[j] * p.A10) * gk) * invz[j];
      }
    } else {
      const float c0 = dn < 0 ? 1.f : p.A01, c1 = dn < 0 ? 1.f : p.A11;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        w0[j] = ring[q].a0[j] * c0;
        w1[j] = ring[q].a1[j] * c1;
      }
    }
    const float u = ring[q].u;
    slot_consumed<J>(w0);
    slot_consumed<J>(w1);
    asm volatile("" ::"v"(u));
    if (refill) samp_row_load<J, VEC>(p, urow, t - PF > t_a ? t - PF : t_a, j0, ring[q]);
    // the lane's sums in latent order, then the wave's inclusive scans
    float s0 = w0[0], s1 = w1[0];
#pragma unroll
    for (int j = 1; j < J; ++j) {
      s0 += w0[j];
      s1 += w1[j];
    }
    float i0 = s0, i1 = s1;
    wave_scan2(lane, i0, i1);
    const float tot0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(i0), 63));
    const float tot1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(i1), 63));
    const float total = tot0 + tot1;
    if (!(total > 0.f) || !(total < INFINITY)) {   // wave-uniform: nothing to draw from
      for (int64_t tt = t_a + lane; tt <= t; tt += 64) {
        pd[tt] = -1;
        pl[tt] = -1;
      }
      bstore_i32_lane0(p.status, 0, 1);
      return false;
    }
    float e0 = __shfl_up(i0, 1, 64), e1 = __shfl_up(i1, 1, 64);
    if (lane == 0) {
      e0 = 0.f;
      e1 = 0.f;
    }
    const float target = u * total;
    const bool p0 = s0 > 0.f, p1 = s1 > 0.f;
    const uint64_t m0 = __ballot(p0 && i0 > target);
    const uint64_t m1 = __ballot(p1 && (tot0 + i1) > target);
    int row, ls;
    if (m0) {
      row = 0;
      ls = __builtin_ctzll(m0);
    } else if (m1) {
      row = 1;
      ls = __builtin_ctzll(m1);
    } else {   // rounding put the target at or past the total: the last state of weight > 0
      const uint64_t q1 = __ballot(p1), q0 = __ballot(p0);
      row = q1 ? 1 : 0;
      ls = 63 - __builtin_clzll(q1 ? q1 : q0);
    }
    // every lane walks its J values of that row; the located lane's answer is taken
    const float base = row ? tot0 + e1 : e0;
    float acc = 0.f;
    int jfirst = -1, jlast = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float w = row ? w1[j] : w0[j];
      acc = j ? acc + w : w;
      const bool pos = w > 0.f;
      if (pos && jfirst < 0 && base + acc > target) jfirst = j;
      if (pos) jlast = j;
    }
    const int jsel = __builtin_amdgcn_readlane(jfirst >= 0 ? jfirst : jlast, ls);
    dn = row;
    ln = ls * J + jsel;
    bstore_i32_lane0(pd, t, dn);
    bstore_i32_lane0(pl, t, ln);
    return true;
  };
  int64_t tb = t_b - 1;
  for (; tb - (PF - 1) >= t_a; tb -= PF) {
#pragma unroll
    for (int q = 0; q < PF; ++q)
      if (!body(q, tb - q, true)) return;
  }
#pragma unroll
  for (int q = 0; q < PF; ++q)
    if (tb - q >= t_a)
      if (!body(q, tb - q, false)) return;
}

template <int J>
__global__ void __launch_bounds__(64) k_segment_sample(SampleParams p) {
  // g[k] for k <= band, zero up to 63: the lookup of a lane's taps
  __shared__ float sg[64];
  {
    const int lane = threadIdx.x & 63;
    float gv = 0.f;
#pragma unroll
    for (int k = 0; k <= kMaxBand; ++k) gv = (lane == k) ? p.g[k] : gv;
    sg[lane] = gv;
    __syncthreads();
  }
  if constexpr (J % 4 == 0) {
    if ((p.L & 3) == 0) {
      seg_sample<J, 1>(p, sg);
      return;
    }
  }
  seg_sample<J, 0>(p, sg);
}

typedef void (*samp_kernel_t)(SampleParams);
static samp_kernel_t samp_kernel(int J) {
  switch (J) {
    case 1: return k_segment_sample<1>;
    case 2: return k_segment_sample<2>;
    case 4: return k_segment_sample<4>;
    case 8: return k_segment_sample<8>;
    case 16: return k_segment_sample<16>;
  }
  return nullptr;
}

}  // namespace pmg

using namespace pmg;

extern "C" {

int pmg_segment_sample(const float* alpha, int64_t T, const int64_t* seg_off, int32_t S, const int32_t* order,
                       const pmg_transition* tr, const float* uniforms, int32_t R, int32_t* path_d,
                       int32_t* path_l, int32_t* status, void* stream) {
  PMG_REQUIRE(T > 0, "pmg_segment_sample: T=%lld must be > 0", (long long)T);
  PMG_REQUIRE(S >= 1, "pmg_segment_sample: S=%d segments (>= 1)", S);
  PMG_REQUIRE(R >= 1, "pmg_segment_sample: R=%d samples (>= 1)", R);
  PMG_REQUIRE((int64_t)S * R <= 0x7fffffffLL, "pmg_segment_sample: S=%d x R=%d workgroups exceed the grid", S, R);
  PMG_REQUIRE(alpha, "pmg_segment_sample: alpha is null");
  PMG_REQUIRE(seg_off, "pmg_segment_sample: seg_off is null");
  const int tr_rc = check_banded_tr("pmg_segment_sample", tr, false);
  if (tr_rc == PMG_EINVAL) return tr_rc;
  PMG_REQUIRE(uniforms, "pmg_segment_sample: uniforms is null");
  PMG_REQUIRE(path_d, "pmg_segment_sample: path_d is null");
  PMG_REQUIRE(path_l, "pmg_segment_sample: path_l is null");
  PMG_REQUIRE(status, "pmg_segment_sample: status is null");
  if (tr_rc) return tr_rc;   // L > 1024
  const int J = pick_J(tr->L);
  SampleParams p;
  memset(&p, 0, sizeof(p));
  p.alpha = alpha;
  p.invz = tr->invz;
  p.uniforms = uniforms;
  p.seg.seg_off = seg_off;
  p.seg.order = order;
  p.seg.S = S;
  p.path_d = path_d;
  p.path_l = path_l;
  p.status = status;
  p.T = T;
  p.L = tr->L;
  p.band = tr->band;
  p.R = R;
  p.A00 = tr->A[0];
  p.A01 = tr->A[1];
  p.A10 = tr->A[2];
  p.A11 = tr->A[3];
  for (int k = 0; k <= kMaxBand; ++k) p.g[k] = (k <= tr->band) ? tr->g[k] : 0.f;
  const samp_kernel_t kf = samp_kernel(J);
  PMG_REQUIRE(kf, "pmg_segment_sample: no kernel for J=%d", J);
  hipLaunchKernelGGL(kf, dim3((unsigned)((int64_t)S * R)), dim3(64), 0, as_stream(stream), p);
  PMG_LAUNCH_CHECK();
  return PMG_OK;
}

}  // extern "C"
