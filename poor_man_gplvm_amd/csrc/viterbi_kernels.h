// Device code of the max-plus (Viterbi) kernels of viterbi.hip.  Every function here works
// on ONE chain (VitChain: its index, its first row and its row count), whether it is one of
// equal-length stacked sequences or a ragged segment: a chain's outputs depend on its own
// rows alone.
//
// The recurrence is filter_one_step (decoder.py:151-172) with each logsumexp replaced
// by a max (the reference has no Viterbi of its own), over the device transition of
// pmg_transition (banded K0, exactly -inf beyond the band; K1 = 1/L):
//   a[d'][i] = max_d (delta_[d][i] + logA[d,d'])
//   v0[j]    = max_{|i-j|<=band} (a[0][i] + log g[|i-j|] + log invz[i])
//   v1       = max_i a[1][i] - log L                      (one scalar and arg-max per step)
//   delta_'[d'][j] = v_d'[j] + s*delta[t,j] + phi[t,j/32]
#pragma once
#include <math.h>
#include <stddef.h>

#include "fb_kernels.h"

namespace pmg {

struct VitParams {
  const float* delta;     // (T, L)
  const float* phi;       // (T, nblk)
  const double* rblk;     // (T, nblk)
  const float* invz;      // (L)
  const double* log_pi0;  // (2, L)
  int64_t T;              // rows of the call, all chains together
  // R: chains in the call.  No kernel reads it: it is padding.  With the tables below 4 bytes
  // earlier, the compiler's register allocation for (J, WP) = (4, 5) and (4, 9) comes out 1-2
  // VGPRs higher and loses a wave of occupancy (seen in the compiler's resource remarks; the
  // reason is not understood).  The static_assert below pins the offset.
  int L, Lpad, nblk, band, R;
  float lg[kMaxBand + 1];  // log g[k] (-inf beyond the band)
  float la[4];             // log A00 A01 A10 A11 (-inf allowed)
  float logL, s;
  double lg64[kMaxBand + 1];
  double la64[4];
  double logL64, s64;
  uint8_t* bp;    // [T][Lpad] back-pointer bytes (row 0 of a chain is not used)
  int32_t* jp;    // [T] jump back-pointers
  int32_t* last;  // [chains][2] the final (d, l)
  double* inc;    // [T] per-step increments of the path score
  int32_t* path_d;
  int32_t* path_l;
  double* log_joint;
};
static_assert(offsetof(VitParams, lg) == 68, "VitParams: see the comment on R before moving lg");

template <int J> constexpr int vit_pf() { return J >= 16 ? 2 : 4; }

template <int J>
struct VitRow {
  RowV<J> d;
  float ph;
};

// A chain: the rows [a, a + len) one wave walks (len >= 1); id: its index in `last` (and
// log_joint).  All three are wave-uniform.
struct VitChain {
  int id;
  int64_t a, len;
};

// row t of the chain whose first emission rows are `delta` / `phi`
template <int J, int VEC>
__device__ __forceinline__ void vit_load(const VitParams& p, const float* delta, const float* phi, int64_t t, int j0,
                                         VitRow<J>& r) {
  bload_row<J, VEC>(delta + t * p.L, p.L, j0, r.d);
  const __amdgpu_buffer_rsrc_t rs = rsrc_of(phi + t * p.nblk, (uint32_t)p.nblk * 4u);
  r.ph = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (j0 >> 5) * 4, 0, 0));
}

// two independent wave maxima (interleaved), each in every lane
__device__ __forceinline__ void wave_max2(float& a, float& b) {
  a = fmaxf(a, dppf<0xB1>(a));
  b = fmaxf(b, dppf<0xB1>(b));
  a = fmaxf(a, dppf<0x4E>(a));
  b = fmaxf(b, dppf<0x4E>(b));
  a = fmaxf(a, dppf<0x141>(a));
  b = fmaxf(b, dppf<0x141>(b));
  a = fmaxf(a, dppf<0x140>(a));
  b = fmaxf(b, dppf<0x140>(b));
  a = fmaxf(a, dppf<0x142, 0xa>(a));
  b = fmaxf(b, dppf<0x142, 0xa>(b));
  a = fmaxf(a, dppf<0x143, 0xc>(a));
  b = fmaxf(b, dppf<0x143, 0xc>(b));
  a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 63));
  b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), 63));
}

// the value `x` of the first lane whose `v` equals the wave maximum `m` (lane 0 if none)
__device__ __forceinline__ int first_at_max(float v, float m, int x) {
  const unsigned long long mask = __ballot(v == m);
  const int ls = mask ? (int)__builtin_ctzll(mask) : 0;
  return __builtin_amdgcn_readlane(x, __builtin_amdgcn_readfirstlane(ls));
}

// out[j] = max_{k=-WP..WP} (in[j+k] + lg[|k|]) over the whole latent line (-inf halo),
// code[j] = k + WP of the maximiser with the smallest k (np.argmax's first index);
// WP (the centre) where every candidate is -inf.
template <int J, int WP>
__device__ __forceinline__ void band_max(const VitParams& p, const float in[J], float out[J], int code[J]) {
  constexpr int NL = (WP + J - 1) / J;  // neighbour lanes on each side
  constexpr int C = NL * J;             // window index of this lane's first latent
  const float ninf = -INFINITY;
  float win[J + 2 * C];
#pragma unroll
  for (int i = 0; i < J; ++i) win[C + i] = in[i];
#pragma unroll
  for (int k = 1; k <= NL; ++k)
#pragma unroll
    for (int i = 0; i < J; ++i) {
      if (k * J - i > WP) win[C - k * J + i] = ninf;
      else win[C - k * J + i] = wave_shr1_in(win[C - (k - 1) * J + i], ninf);
    }
#pragma unroll
  for (int k = 1; k <= NL; ++k)
#pragma unroll
    for (int i = 0; i < J; ++i) {
      if (k * J + i - (J - 1) > WP) win[C + k * J + i] = ninf;
      else win[C + k * J + i] = wave_shl1_in(win[C + (k - 1) * J + i], ninf);
    }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    float best = ninf;
    int bc = WP;
#pragma unroll
    for (int k = -WP; k <= WP; ++k) {
      const float c = win[C + j + k] + p.lg[k < 0 ? -k : k];
      const bool gt = c > best;
      best = gt ? c : best;
      bc = gt ? (k + WP) : bc;
    }
    out[j] = best;
    code[j] = bc;
  }
}

// J back-pointer bytes of one lane, row `row` (Lpad bytes: every lane is in range)
template <int J>
__device__ __forceinline__ void store_codes(uint8_t* row, int Lpad, int j0, const uint32_t b[J]) {
  const __amdgpu_buffer_rsrc_t rs = rsrc_of(row, (uint32_t)Lpad);
  if constexpr (J == 1) {
    __builtin_amdgcn_raw_buffer_store_b8((unsigned char)b[0], rs, j0, 0, 0);
  } else if constexpr (J == 2) {
    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(b[0] | (b[1] << 8)), rs, j0, 0, 0);
  } else {
    uint32_t w[J / 4];
#pragma unroll
    for (int i = 0; i < J / 4; ++i) w[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24);
    if constexpr (J == 4) {
      __builtin_amdgcn_raw_buffer_store_b32(w[0], rs, j0, 0, 0);
    } else if constexpr (J == 8) {
      const u32x2 q = {w[0], w[1]};
      __builtin_amdgcn_raw_buffer_store_b64(q, rs, j0, 0, 0);
    } else {
      static_assert(J == 16, "lane layouts: J in {1, 2, 4, 8, 16}");
      const u32x4 q = {w[0], w[1], w[2], w[3]};
      __builtin_amdgcn_raw_buffer_store_b128(q, rs, j0, 0, 0);
    }
  }
}

// The forward scan of one chain by one wave; last[2 id ..] receives the final (d, l).
// Every ring address is clamped to the chain's own last row, and rows 1 .. n-1 of its bp /
// jp are written (row 0 has no back-pointers): no access leaves the chain's rows.
template <int J, int WP, int VEC>
__device__ __forceinline__ void vit_forward(const VitParams& p, const VitChain& ch) {
  constexpr int PF = vit_pf<J>();
  const float ninf = -INFINITY;
  const int j0 = (int)threadIdx.x * J;
  const float* delta = p.delta + ch.a * p.L;
  const float* phi = p.phi + ch.a * p.nblk;
  uint8_t* bp = p.bp + ch.a * p.Lpad;
  int32_t* jp = p.jp + ch.a;
  const int shift = WP - p.band;   // code of band_max -> i - j + band

  bool ok[J];
  float linvz[J], d0[J], d1[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    ok[j] = j0 + j < p.L;
    linvz[j] = ok[j] ? (float)log((double)p.invz[j0 + j]) : ninf;
  }
  {  // t = 0: the filter's own prior, centred by its maximum in f64 before it is rounded
     // to f32 (pi0[0, j] and pi0[1, j] differ by ~1e-8 relative in the interior)
    VitRow<J> r0;
    vit_load<J, VEC>(p, delta, phi, 0, j0, r0);
    double lp0[J], lp1[J];
    double c0 = -INFINITY;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      lp0[j] = ok[j] ? p.log_pi0[j0 + j] : (double)-INFINITY;
      lp1[j] = ok[j] ? p.log_pi0[p.L + j0 + j] : (double)-INFINITY;
      c0 = fmax(c0, fmax(lp0[j], lp1[j]));
    }
    c0 = wave_max_f64(c0);
    if (!(c0 > -1.0e300)) c0 = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float em = fmaf(p.s, r0.d[j], r0.ph);
      d0[j] = ok[j] ? (float)(lp0[j] - c0) + em : ninf;
      d1[j] = ok[j] ? (float)(lp1[j] - c0) + em : ninf;
    }
  }
  if (ch.len > 1) {
    const int64_t last = ch.len - 1;
    VitRow<J> ring[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) vit_load<J, VEC>(p, delta, phi, 1 + q < last ? 1 + q : last, j0, ring[q]);
    auto body = [&](int q, int64_t t, bool refill) {
      float em[J];
      order_after(ring[q].ph, d0[0]);
#pragma unroll
      for (int j = 0; j < J; ++j) em[j] = fmaf(p.s, ring[q].d[j], ring[q].ph);
      slot_consumed<J>(em);
      if (refill) vit_load<J, VEC>(p, delta, phi, t + PF < last ? t + PF : last, j0, ring[q]);
      // dynamics mix; the lane's best jump predecessor (first index on ties)
      float a0[J];
      uint32_t b0[J];
      float m0 = ninf, lv = ninf;
      int li = j0, lb = 0;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const float x = d0[j] + p.la[0], y = d1[j] + p.la[2];
        const bool by = y > x;
        a0[j] = by ? y : x;
        b0[j] = by ? 0x80u : 0u;
        m0 = fmaxf(m0, a0[j]);
        const float u = d0[j] + p.la[1], w = d1[j] + p.la[3];
        const bool bw = w > u;
        const float a1 = bw ? w : u;
        const bool gt = a1 > lv;
        lv = gt ? a1 : lv;
        li = gt ? j0 + j : li;
        lb = gt ? (bw ? 1 : 0) : lb;
      }
      float M0 = m0, M1 = lv;
      wave_max2(M0, M1);
      const int jw = first_at_max(lv, M1, li | (lb << 16));
      float c = fmaxf(M0, M1);
      if (!(c > -3.0e38f)) c = 0.f;
      float ain[J], v0[J];
      int code[J];
#pragma unroll
      for (int j = 0; j < J; ++j) ain[j] = a0[j] + linvz[j];
      band_max<J, WP>(p, ain, v0, code);
      const float v1 = (M1 - p.logL) - c;
      uint32_t bytes[J];
#pragma unroll
      for (int j = 0; j < J; ++j) {
        d0[j] = ok[j] ? (v0[j] - c) + em[j] : ninf;
        d1[j] = ok[j] ? v1 + em[j] : ninf;
        bytes[j] = (uint32_t)(code[j] - shift) | b0[j];
      }
      store_codes<J>(bp + t * p.Lpad, p.Lpad, j0, bytes);
      const __amdgpu_buffer_rsrc_t rs = rsrc_of(jp + t, 4u);
      __builtin_amdgcn_raw_buffer_store_b32((uint32_t)jw, rs, threadIdx.x == 0 ? 0 : 64, 0, 0);
    };
    int64_t tb = 1;
    for (; tb + PF <= ch.len; tb += PF) {
#pragma unroll
      for (int q = 0; q < PF; ++q) body(q, tb + q, true);
    }
#pragma unroll
    for (int q = 0; q < PF; ++q)
      if (tb + q < ch.len) body(q, tb + q, false);
  }
  // the final state: argmax over the flattened (2, L) scores (first index on ties)
  float l0 = ninf, l1 = ninf;
  int i0 = j0, i1 = j0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const bool g0 = d0[j] > l0, g1 = d1[j] > l1;
    l0 = g0 ? d0[j] : l0;
    i0 = g0 ? j0 + j : i0;
    l1 = g1 ? d1[j] : l1;
    i1 = g1 ? j0 + j : i1;
  }
  float M0 = l0, M1 = l1;
  wave_max2(M0, M1);
  const int e0 = first_at_max(l0, M0, i0), e1 = first_at_max(l1, M1, i1);
  if (threadIdx.x == 0) {
    const bool jump = M1 > M0;
    p.last[2 * ch.id] = jump ? 1 : 0;
    p.last[2 * ch.id + 1] = jump ? e1 : e0;
  }
}

// Back-trace of one chain by one wave.  A piece is NP = min(64, 16384 / Lpad) consecutive
// rows of the chain, counted from its first row (<= 16 KiB, <= 16 16-byte loads per lane);
// lane s of the wave keeps step s of the piece, so the path leaves in one coalesced store
// per piece.  The chain's first back-pointer row is 16-byte aligned (Lpad is a multiple of
// 64); the 16-byte loads are clamped to the chain's own last 16-byte group and the jp loads
// to its last row.  Uses 16.25 KiB of the workgroup's LDS.
constexpr int kTracePieceBytes = 16384;
__device__ __forceinline__ void vit_trace(const VitParams& p, const VitChain& ch) {
  __shared__ __attribute__((aligned(16))) uint8_t rows[kTracePieceBytes];
  __shared__ int32_t jrow[64];
  const int lane = threadIdx.x;
  const int Lpad = p.Lpad;
  const int NP = kTracePieceBytes / Lpad < 64 ? kTracePieceBytes / Lpad : 64;
  const int nv = NP * Lpad / 1024;
  const int64_t n = ch.len;
  const int64_t row0 = ch.a;
  const uint8_t* bp = p.bp + row0 * Lpad;
  const int32_t* jp = p.jp + row0;
  const int64_t end = n * Lpad - 16;   // the last 16-byte group of this chain's rows
  const int64_t npiece = (n + NP - 1) / NP;
  u32x4 regs[16];
  int32_t jreg = 0;
  auto load_piece = [&](int64_t pc) {
    const int64_t base = pc * NP;
#pragma unroll
    for (int v = 0; v < 16; ++v)
      if (v < nv) {
        int64_t off = base * Lpad + v * 1024 + lane * 16;
        off = off < end ? off : end;
        regs[v] = *reinterpret_cast<const u32x4*>(bp + off);
      }
    const int64_t tj = base + lane < n ? base + lane : n - 1;
    jreg = jp[tj];
  };
  int d = p.last[2 * ch.id], l = p.last[2 * ch.id + 1];
  d = __builtin_amdgcn_readfirstlane(d);
  l = __builtin_amdgcn_readfirstlane(l);
  load_piece(npiece - 1);
  for (int64_t pc = npiece - 1; pc >= 0; --pc) {
    const int64_t base = pc * NP;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 16; ++v)
      if (v < nv) *reinterpret_cast<u32x4*>(rows + v * 1024 + lane * 16) = regs[v];
    jrow[lane] = jreg;
    __syncthreads();
    if (pc > 0) load_piece(pc - 1);
    const int s_hi = (int)((base + NP < n ? base + NP : n) - base) - 1;
    int myd = 0, myl = 0;
    for (int s = s_hi; s >= 0; --s) {
      myd = lane == s ? d : myd;
      myl = lane == s ? l : myl;
      if (base + s == 0) break;
      if (d == 1) {
        const int w = __builtin_amdgcn_readfirstlane(jrow[s]);
        l = w & 0xffff;
        d = (w >> 16) & 1;
      } else {
        const int code = __builtin_amdgcn_readfirstlane((int)rows[s * Lpad + l]);
        int i = l + (code & 127) - p.band;
        i = i < 0 ? 0 : (i > p.L - 1 ? p.L - 1 : i);
        d = __builtin_amdgcn_readfirstlane((int)rows[s * Lpad + i]) >> 7;
        l = i;
      }
      l = l > p.L - 1 ? p.L - 1 : l;
    }
    if (lane <= s_hi) {
      p.path_d[row0 + base + lane] = myd;
      p.path_l[row0 + base + lane] = myl;
    }
  }
}

// inc[idx] = the increment of log p(x, y) at global row idx along the path, f64; `first`:
// the row is its chain's first (the prior term; otherwise the transition from row
// idx - 1).  NaN for an out-of-range path entry.
__device__ __forceinline__ void vit_increment(const VitParams& p, int64_t idx, bool first) {
  const int d = p.path_d[idx], l = p.path_l[idx];
  if ((unsigned)d > 1u || (unsigned)l >= (unsigned)p.L) {
    p.inc[idx] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const double ll = p.rblk[idx * p.nblk + (l >> 5)] + (double)p.delta[idx * p.L + l];
  double v = p.s64 * ll;
  if (first) {
    v += p.log_pi0[d * p.L + l];
  } else {
    const int dp = p.path_d[idx - 1] & 1;
    int lp = p.path_l[idx - 1];
    lp = lp < 0 ? 0 : (lp > p.L - 1 ? p.L - 1 : lp);
    v += p.la64[dp * 2 + d];
    if (d == 0) {
      const int k = l > lp ? l - lp : lp - l;
      v += (k <= p.band ? p.lg64[k] : (double)-INFINITY) + log((double)p.invz[lp]);
    } else {
      v -= p.logL64;
    }
  }
  p.inc[idx] = v;
}

// sum_t inc[t], t = 0 .. n-1, by one workgroup of 256 threads: thread i adds steps i,
// i + 256, ... in order, then a fixed tree over the 256 partial sums (`part`: 256 doubles
// of LDS).  The order depends on n alone.  The result is valid in thread 0.
__device__ __forceinline__ double vit_sum(const double* inc, int64_t n, double* part) {
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int64_t t = tid; t < n; t += 256) a += inc[t];
  part[tid] = a;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) part[tid] += part[tid + h];
    __syncthreads();
  }
  return part[0];
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// the transition's logs (f32 for the scan, f64 for the score), the shape and the scale;
// the caller sets the emission, workspace and output pointers, T and R
static void vit_fill_params(VitParams& p, const pmg_transition* tr, int J, double likelihood_scale) {
  memset(&p, 0, sizeof(p));
  p.invz = tr->invz;
  p.L = tr->L;
  p.Lpad = 64 * J;
  p.nblk = (int)(round_up(tr->L, 32) / 32);
  p.band = tr->band;
  for (int k = 0; k <= kMaxBand; ++k) {
    p.lg64[k] = (k <= tr->band && tr->g[k] > 0.f) ? log((double)tr->g[k]) : -INFINITY;
    p.lg[k] = (float)p.lg64[k];
  }
  for (int k = 0; k < 4; ++k) {
    p.la64[k] = tr->A[k] > 0.f ? log((double)tr->A[k]) : -INFINITY;
    p.la[k] = (float)p.la64[k];
  }
  p.logL64 = log((double)tr->L);
  p.logL = (float)p.logL64;
  p.s64 = likelihood_scale;
  p.s = (float)likelihood_scale;
}

}  // namespace pmg
