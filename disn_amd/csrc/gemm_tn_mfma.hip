// Weight-gradient GEMM ("TN"): C[P][Q] = sum_m A[m][p] * B[m][q], reduction over the ROWS of two
// row-major activations -- dW = X^T dZ of a 1x1 conv (models/sdfnet.py layers) or, with implicit
// im2col, of a 3x3 SAME conv (models/CNN/vgg.py:187-196): p = tap*Cin + ci, A[m][p] = X at pixel m
// shifted by the tap (zero outside the image).  Training step of SURVEY 8f #3.
//
// fp32 MFMA (v_mfma_f32_32x32x2_f32); BP x BQ output tile per workgroup (64 or 128 each), 4 waves
// 2x2, (BP/64)x(BQ/64) 32x32 accumulators per wave; the reduction advances 32 rows per step.  Both
// operands are staged through LDS as [32 rows][BP | BQ cols] row-major copies of global memory
// (coalesced float4 loads); an MFMA fragment wants 32 consecutive COLUMNS of one row per half-wave,
// i.e. consecutive LDS words (row stride padded by 8 words so the two half-waves, 4 rows apart, use
// disjoint banks): conflict-free ds_read_b32.  k-permutation as in gemm_mfma.hip: MFMA k-index h of
// step t inside an 8-row block is row 4h + t on both operands.
// A 128x128 tile moves 32 KB per 1 MFLOP (64x64: 16 KB per 0.26 MFLOP): the 64x64 version of this
// kernel was L2-bandwidth bound at 77 TFLOP/s.
// The output is small (<= 4608 x 512) and the reduction long (2k .. 400k rows), so the work is
// ALWAYS stream-K: (tile, row-step) units split evenly over W workgroups; a segment that covers a
// whole tile is finished in place, any other goes to a slab and tn_fixup sums the slabs of a tile in
// workgroup order (deterministic, no atomics).
#include "kernels.hpp"
#include "h2_common.hpp"

#include <type_traits>

namespace disn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct TnDev {
  TnParams p;
  float* ws;  // slabs [2*W][BP*BQ]
  int msteps, ptiles, qtiles, W;
  long units;
  int kt;  // > 0: INTERLEAVED reduction -- workgroup w = tile (w % T), row steps (w / T) + i kt: all workgroups walk the
           // rows of A and B together, a window of 32 kt rows at a time (L2-resident), instead of each streaming its own
           // contiguous range; one slab per workgroup, tn_fixup sums a tile's kt slabs in order
};

__device__ __forceinline__ long tn_unit_begin(long U, int W, int w) { return (U * w) / W; }

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// BF: the multiply on the bf16 MFMA (v_mfma_f32_32x32x16_bf16, mixed-precision step).  Both operands
// are then staged TRANSPOSED, as bf16 T[col][32 m] rows of 40 (80 bytes), so that a fragment -- 8
// consecutive m of one column -- is one conflict-free ds_read_b128.  The transposing LDS write is a
// ds_write_b32 of the bf16 pair (m, m+1): a thread loads the same float4 column group of two adjacent
// rows; lanes of a 32-lane write group are 16 row pairs x 2 column groups = 32 distinct banks.
// MODE 2 (round 3): the fp32-ACCURATE multiply on the f16 pipes -- both operands as two-term f16 splits (h + l of
// v * 2^k, k from the operand's maximum: TnParams::amax_a / amax_b), l_a h_b + h_a l_b + h_a h_b on
// v_mfma_f32_32x32x16_f16, as conv_h2.hip does for the forward.  Same transposed staging as the bf16 form with two
// planes per operand (80 KiB of LDS for the 128 x 128 tile's two stages), and the global loads run TWO row steps
// ahead (two register sets): the step loop of the bf16 form waits a full memory latency per 8 MFMAs.
template <int BP, int BQ, bool CONV, int MODE>
__global__ __launch_bounds__(256, 2) void gemm_tn_f32_mfma(const TnDev d) {
  constexpr bool BF = MODE == 1;
  constexpr int LDP = BP + 8, LDQ = BQ + 8;      // padded LDS row strides (words)
  constexpr int BUF = 32 * (LDP + LDQ);          // one stage
  constexpr int TP = BP / 64, TQ = BQ / 64;      // 32x32 accumulators per wave, per dimension
  constexpr int AV = BP / 4, BV = BQ / 4;        // float4 per operand row
  constexpr int AROWS = 256 / AV, BROWS = 256 / BV;  // rows one loader pass covers
  constexpr int APASS = 32 / AROWS, BPASS = 32 / BROWS;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const TnParams& p = d.p;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int w = xcd_tile(d.W, blockIdx.x);
  const int MS = d.msteps;
  const int KT = d.kt;
  if (KT > 0) w = blockIdx.x;
  const long u0 = KT > 0 ? 0 : tn_unit_begin(d.units, d.W, w), u1 = KT > 0 ? 1 : tn_unit_begin(d.units, d.W, w + 1);

  for (long u = u0; u < u1;) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));  // keep lane-dependent addressing inside the segment loop
    const int lane = tid & 63;
    int tile, s_begin, s_end, slot;
    const int sstep = KT > 0 ? KT : 1;
    if (KT > 0) {
      const int T = d.ptiles * d.qtiles;
      tile = w % T;
      s_begin = w / T;
      s_end = MS;
      slot = w;
      u = u1;
    } else {
      tile = (int)(u / MS);
      s_begin = (int)(u - (long)tile * MS);
      const long rest = u1 - (long)tile * MS;
      s_end = rest < MS ? (int)rest : MS;
      slot = (u == u0) ? 2 * w : 2 * w + 1;
      u += s_end - s_begin;
    }
    const int pt = tile / d.qtiles, qt = tile - pt * d.qtiles;
    const int p0 = pt * BP, q0 = qt * BQ;
    f32x16 acc[TP][TQ];
#pragma unroll
    for (int i = 0; i < TP; ++i)
#pragma unroll
      for (int j = 0; j < TQ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float descale = 1.0f;
    if constexpr (MODE == 2) {
      // ---------------- two-term f16 path ----------------
      constexpr int LDT = 40;                          // f16 per transposed row (32 m + pad): 80 bytes
      constexpr int TBUF = 2 * (BP + BQ) * LDT;        // one stage: A_h, A_l, B_h, B_l
      constexpr int PA = BP / 64, PB = BQ / 64;
      _Float16* tl = reinterpret_cast<_Float16*>(lds);
      const int rp = tid & 15, cg = tid >> 4;
      float sa, sb;
      {
        float ma = 0.f, mb = 0.f;
        for (int k = lane; k < p.amax_a_n; k += 64) ma = fmaxf(ma, p.amax_a[k]);
        for (int k = lane; k < p.amax_b_n; k += 64) mb = fmaxf(mb, p.amax_b[k]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          ma = fmaxf(ma, __shfl_xor(ma, off));
          mb = fmaxf(mb, __shfl_xor(mb, off));
        }
        sa = ch2::pow2_scale(ma, 14);
        sb = ch2::pow2_scale(mb, 14);
        descale = (1.0f / sa) * (1.0f / sb);
      }
      int tdy[PA], tdx[PA], tci[PA];
#pragma unroll
      for (int q = 0; q < PA; ++q) {
        const int col = p0 + 4 * (cg + 16 * q);
        tdy[q] = 0; tdx[q] = 0; tci[q] = col;
        if (CONV) {
          const int tap = col / p.Cin;
          tci[q] = col - tap * p.Cin;
          tdy[q] = tap / 3 - 1;
          tdx[q] = tap - (tap / 3) * 3 - 1;
        }
      }
      float4 xa[2][PA][2], xb[2][PB][2];
      auto load = [&](int s, auto set_c) {
        constexpr int SET = decltype(set_c)::value;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const long m = (long)s * 32 + 2 * rp + h;
          const bool okm = m < p.M;
          const long mm = okm ? m : 0;
          int y = 0, x = 0;
          if (CONV) {
            const int hw = p.H * p.W;
            const int rem = (int)(mm % hw);
            y = rem / p.W;
            x = rem - y * p.W;
          }
#pragma unroll
          for (int q = 0; q < PA; ++q) {
            bool ok = okm;
            const float* src;
            if (CONV) {
              const int yy = y + tdy[q], xx = x + tdx[q];
              ok = ok && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
              src = p.a + (size_t)(ok ? mm + tdy[q] * p.W + tdx[q] : 0) * p.Cin + tci[q];
            } else {
              src = p.a + (size_t)mm * p.lda + tci[q];
            }
            const float4 v = *reinterpret_cast<const float4*>(src);
            xa[SET][q][h] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int q = 0; q < PB; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(p.b + (size_t)mm * p.ldb + q0 + 4 * (cg + 16 * q));
            xb[SET][q][h] = okm ? v : make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
      };
      typedef _Float16 h2v __attribute__((ext_vector_type(2)));
      // rows (m, m + 1) of four columns: per column one f16 pair into the h plane, one into the l plane
      auto put = [&](_Float16* th, _Float16* tlo, int colbase, const float4& lo, const float4& hi, float sc) {
        const float l4[4] = {lo.x, lo.y, lo.z, lo.w}, h4[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v0 = l4[j] * sc, v1 = h4[j] * sc;
          h2v vh, vl;
          vh[0] = (_Float16)v0;
          vh[1] = (_Float16)v1;
          vl[0] = (_Float16)(v0 - (float)vh[0]);
          vl[1] = (_Float16)(v1 - (float)vh[1]);
          *reinterpret_cast<h2v*>(&th[(colbase + j) * LDT + 2 * rp]) = vh;
          *reinterpret_cast<h2v*>(&tlo[(colbase + j) * LDT + 2 * rp]) = vl;
        }
      };
      auto store = [&](int buf, auto set_c) {
        constexpr int SET = decltype(set_c)::value;
        _Float16* ta = tl + buf * TBUF;
        _Float16* tb = ta + 2 * BP * LDT;
#pragma unroll
        for (int q = 0; q < PA; ++q) put(ta, ta + BP * LDT, 4 * (cg + 16 * q), xa[SET][q][0], xa[SET][q][1], sa);
#pragma unroll
        for (int q = 0; q < PB; ++q) put(tb, tb + BQ * LDT, 4 * (cg + 16 * q), xb[SET][q][0], xb[SET][q][1], sb);
      };
      auto compute = [&](int cur) {
        const _Float16* ta = tl + cur * TBUF + (wm * (BP / 2) + (lane & 31)) * LDT + 8 * (lane >> 5);
        const _Float16* tb = tl + cur * TBUF + 2 * BP * LDT + (wn * (BQ / 2) + (lane & 31)) * LDT + 8 * (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          ch_h8 ah[TP], al[TP], bh[TQ], bl[TQ];
#pragma unroll
          for (int i = 0; i < TP; ++i) {
            ah[i] = *reinterpret_cast<const ch_h8*>(ta + i * 32 * LDT + kk * 16);
            al[i] = *reinterpret_cast<const ch_h8*>(ta + BP * LDT + i * 32 * LDT + kk * 16);
          }
#pragma unroll
          for (int j = 0; j < TQ; ++j) {
            bh[j] = *reinterpret_cast<const ch_h8*>(tb + j * 32 * LDT + kk * 16);
            bl[j] = *reinterpret_cast<const ch_h8*>(tb + BQ * LDT + j * 32 * LDT + kk * 16);
          }
#pragma unroll
          for (int i = 0; i < TP; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
          for (int i = 0; i < TP; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
          for (int i = 0; i < TP; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
      };
      const int nsteps = (s_end - s_begin + sstep - 1) / sstep;
      auto S = [&](int i) { return s_begin + (i < nsteps ? i : nsteps - 1) * sstep; };
      using std::integral_constant;
      load(S(0), integral_constant<int, 0>{});
      load(S(1), integral_constant<int, 1>{});
      store(0, integral_constant<int, 0>{});
      __syncthreads();
      int cur = 0;
      for (int i = 0; i < nsteps; i += 2) {
        // step i is in buffer cur, register set 1 holds step i + 1, set 0 is free
        load(S(i + 2), integral_constant<int, 0>{});
        compute(cur);
        store(cur ^ 1, integral_constant<int, 1>{});
        __syncthreads();
        cur ^= 1;
        if (i + 1 >= nsteps) break;
        load(S(i + 3), integral_constant<int, 1>{});
        compute(cur);
        store(cur ^ 1, integral_constant<int, 0>{});
        __syncthreads();
        cur ^= 1;
      }
    } else if constexpr (BF) {
      // ---------------- bf16 path ----------------
      constexpr int LDT = 40;                          // bf16 per transposed row (32 m + pad)
      constexpr int TBUF = (BP + BQ) * LDT;            // one stage, in bf16
      constexpr int PA = BP / 64, PB = BQ / 64;        // loader passes: 16 column groups x 16 row pairs each
      __bf16* tl = reinterpret_cast<__bf16*>(lds);
      const int rp = tid & 15, cg = tid >> 4;          // row pair, column group (4 per wave)
      int tdy[PA], tdx[PA], tci[PA];
#pragma unroll
      for (int q = 0; q < PA; ++q) {
        const int col = p0 + 4 * (cg + 16 * q);
        tdy[q] = 0; tdx[q] = 0; tci[q] = col;
        if (CONV) {
          const int tap = col / p.Cin;
          tci[q] = col - tap * p.Cin;
          tdy[q] = tap / 3 - 1;
          tdx[q] = tap - (tap / 3) * 3 - 1;
        }
      }
      float4 xa[PA][2], xb[PB][2];
      auto load = [&](int s) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const long m = (long)s * 32 + 2 * rp + h;
          const bool okm = m < p.M;
          const long mm = okm ? m : 0;
          int y = 0, x = 0;
          if (CONV) {
            const int hw = p.H * p.W;
            const int rem = (int)(mm % hw);
            y = rem / p.W;
            x = rem - y * p.W;
          }
#pragma unroll
          for (int q = 0; q < PA; ++q) {
            bool ok = okm;
            const float* src;
            if (CONV) {
              const int yy = y + tdy[q], xx = x + tdx[q];
              ok = ok && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
              src = p.a + (size_t)(ok ? mm + tdy[q] * p.W + tdx[q] : 0) * p.Cin + tci[q];
            } else {
              src = p.a + (size_t)mm * p.lda + tci[q];
            }
            const float4 v = *reinterpret_cast<const float4*>(src);
            xa[q][h] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int q = 0; q < PB; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(p.b + (size_t)mm * p.ldb + q0 + 4 * (cg + 16 * q));
            xb[q][h] = okm ? v : make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
      };
      auto put = [&](__bf16* t, int colbase, const float4& lo, const float4& hi) {
        const float l4[4] = {lo.x, lo.y, lo.z, lo.w}, h4[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bf16x2 v;
          v[0] = (__bf16)l4[j];
          v[1] = (__bf16)h4[j];
          *reinterpret_cast<bf16x2*>(&t[(colbase + j) * LDT + 2 * rp]) = v;
        }
      };
      auto store = [&](int buf) {
        __bf16* ta = tl + buf * TBUF;
        __bf16* tb = ta + BP * LDT;
#pragma unroll
        for (int q = 0; q < PA; ++q) put(ta, 4 * (cg + 16 * q), xa[q][0], xa[q][1]);
#pragma unroll
        for (int q = 0; q < PB; ++q) put(tb, 4 * (cg + 16 * q), xb[q][0], xb[q][1]);
      };
      load(s_begin);
      store(0);
      __syncthreads();
      int cur = 0;
      for (int s = s_begin; s < s_end; s += sstep) {
        const int sn = (s + sstep < s_end) ? s + sstep : s;
        load(sn);
        const __bf16* ta = tl + cur * TBUF + (wm * (BP / 2) + (lane & 31)) * LDT + 8 * (lane >> 5);
        const __bf16* tb = tl + cur * TBUF + BP * LDT + (wn * (BQ / 2) + (lane & 31)) * LDT + 8 * (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          bf16x8 af[TP], bfr[TQ];
#pragma unroll
          for (int i = 0; i < TP; ++i) af[i] = *reinterpret_cast<const bf16x8*>(ta + i * 32 * LDT + kk * 16);
#pragma unroll
          for (int j = 0; j < TQ; ++j) bfr[j] = *reinterpret_cast<const bf16x8*>(tb + j * 32 * LDT + kk * 16);
#pragma unroll
          for (int i = 0; i < TP; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        store(cur ^ 1);
        __syncthreads();
        cur ^= 1;
      }
    } else {
    // ---------------- fp32 path ----------------
    // loaders: thread -> float4 column (tid % AV), rows (tid / AV) + AROWS*i
    const int arow = tid / AV, acol = (tid % AV) * 4;
    const int brow = tid / BV, bcol = (tid % BV) * 4;
    // conv: the tap / channel of THIS thread's A column (a P tile may span taps)
    int dy = 0, dx = 0, ci = p0 + acol;
    if (CONV) {
      const int tap = (p0 + acol) / p.Cin;
      ci = p0 + acol - tap * p.Cin;
      dy = tap / 3 - 1;
      dx = tap - (tap / 3) * 3 - 1;
    }
    float4 ra[APASS], rb[BPASS];
    auto load = [&](int s) {
#pragma unroll
      for (int i = 0; i < APASS; ++i) {
        const long m = (long)s * 32 + arow + AROWS * i;
        bool ok = m < p.M;
        const float* src;
        if (CONV) {
          const int hw = p.H * p.W;
          const long mm = ok ? m : 0;
          const int rem = (int)(mm % hw);
          const int y = rem / p.W, x = rem - y * p.W;
          const int yy = y + dy, xx = x + dx;
          ok = ok && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
          src = p.a + (size_t)(ok ? mm + dy * p.W + dx : 0) * p.Cin + ci;
        } else {
          src = p.a + (size_t)(ok ? m : 0) * p.lda + ci;
        }
        const float4 v = *reinterpret_cast<const float4*>(src);
        ra[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < BPASS; ++i) {
        const long m = (long)s * 32 + brow + BROWS * i;
        const bool ok = m < p.M;
        const float4 v = *reinterpret_cast<const float4*>(p.b + (size_t)(ok ? m : 0) * p.ldb + q0 + bcol);
        rb[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    auto store = [&](int buf) {
      float* la = &lds[buf * BUF];
      float* lb = la + 32 * LDP;
#pragma unroll
      for (int i = 0; i < APASS; ++i)
        *reinterpret_cast<float4*>(&la[(arow + AROWS * i) * LDP + acol]) = ra[i];
#pragma unroll
      for (int i = 0; i < BPASS; ++i)
        *reinterpret_cast<float4*>(&lb[(brow + BROWS * i) * LDQ + bcol]) = rb[i];
    };
    load(s_begin);
    store(0);
    __syncthreads();
    int cur = 0;
    for (int s = s_begin; s < s_end; s += sstep) {
      const int sn = (s + sstep < s_end) ? s + sstep : s;
      load(sn);
      const float* la = &lds[cur * BUF] + wm * (BP / 2) + (lane & 31);
      const float* lb = &lds[cur * BUF] + 32 * LDP + wn * (BQ / 2) + (lane & 31);
      const int hrow = (lane >> 5) * 4;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float a[TP], b[TQ];
#pragma unroll
          for (int i = 0; i < TP; ++i) a[i] = la[(kb * 8 + hrow + t) * LDP + i * 32];
#pragma unroll
          for (int j = 0; j < TQ; ++j) b[j] = lb[(kb * 8 + hrow + t) * LDQ + j * 32];
#pragma unroll
          for (int i = 0; i < TP; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
      }
      store(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
    }  // fp32 path
    const bool whole = s_begin == 0 && s_end == MS && sstep == 1;
    float* slab = d.ws + (size_t)slot * BP * BQ;  // tile-local row-major [BP][BQ]
#pragma unroll
    for (int i = 0; i < TP; ++i)
#pragma unroll
      for (int j = 0; j < TQ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * (BP / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const int col = wn * (BQ / 2) + j * 32 + (lane & 31);
          if (whole) {  // the whole reduction of this tile: finish in place (tn_fixup skips it)
            const size_t o = (size_t)(p0 + row) * p.ldc + q0 + col;
            float v = acc[i][j][r] * descale;
            if (p.l2 != 0.f) v += p.l2 * p.wcur[o];
            p.c[o] = v;
          } else {
            slab[row * BQ + col] = acc[i][j][r] * descale;
          }
        }
    if (u < u1) __syncthreads();
  }
}

// C[p][q] = sum of the slabs of tile (pt,qt) in workgroup order, + l2 * Wcur[p][q]
template <int BP, int BQ>
__global__ __launch_bounds__(256) void tn_fixup(const TnDev d) {
  const TnParams& p = d.p;
  const int tile = blockIdx.x;
  if (d.kt > 0) {  // interleaved reduction: slabs tile + T k, k = 0 .. kt - 1
    if (d.kt == 1) return;
    const int T = d.ptiles * d.qtiles;
    const int idx4 = blockIdx.y * 256 + threadIdx.x;
    const int lrow = idx4 / (BQ / 4), lcol = (idx4 - lrow * (BQ / 4)) * 4;
    const float* base = d.ws + (size_t)lrow * BQ + lcol;
    const size_t slab = (size_t)BP * BQ;
    float4 v = *reinterpret_cast<const float4*>(base + (size_t)tile * slab);
    for (int k = 1; k < d.kt; ++k) {
      const float4 u = *reinterpret_cast<const float4*>(base + (size_t)(tile + T * k) * slab);
      v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    const int pt = tile / d.qtiles, qt = tile - pt * d.qtiles;
    const size_t o = (size_t)(pt * BP + lrow) * p.ldc + qt * BQ + lcol;
    if (p.l2 != 0.f) {
      const float4 wv = *reinterpret_cast<const float4*>(p.wcur + o);
      v.x += p.l2 * wv.x; v.y += p.l2 * wv.y; v.z += p.l2 * wv.z; v.w += p.l2 * wv.w;
    }
    *reinterpret_cast<float4*>(p.c + o) = v;
    return;
  }
  const long MS = d.msteps, tb = (long)tile * MS, te = tb + MS;
  int w = (int)((tb * d.W) / d.units);
  while (w + 1 < d.W && tn_unit_begin(d.units, d.W, w + 1) <= tb) ++w;
  while (w > 0 && tn_unit_begin(d.units, d.W, w) > tb) --w;
  int w_last = (int)(((te - 1) * d.W) / d.units);
  while (w_last + 1 < d.W && tn_unit_begin(d.units, d.W, w_last + 1) <= te - 1) ++w_last;
  while (w_last > 0 && tn_unit_begin(d.units, d.W, w_last) > te - 1) --w_last;
  if (w == w_last) return;  // one workgroup reduced the whole tile and wrote it in place
  const int idx4 = blockIdx.y * 256 + threadIdx.x;
  const int lrow = idx4 / (BQ / 4), lcol = (idx4 - lrow * (BQ / 4)) * 4;
  const float* base = d.ws + (size_t)lrow * BQ + lcol;
  const size_t slab = (size_t)BP * BQ;
  const int first_slot = (tn_unit_begin(d.units, d.W, w) >= tb) ? 2 * w : 2 * w + 1;
  float4 v = *reinterpret_cast<const float4*>(base + (size_t)first_slot * slab);
#pragma unroll 4
  for (int k = w + 1; k <= w_last; ++k) {
    const float4 u = *reinterpret_cast<const float4*>(base + (size_t)(2 * k) * slab);
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  const int pt = tile / d.qtiles, qt = tile - pt * d.qtiles;
  const size_t o = (size_t)(pt * BP + lrow) * p.ldc + qt * BQ + lcol;
  if (p.l2 != 0.f) {  // d(wd*|w|^2/2)/dw = wd * w
    const float4 wv = *reinterpret_cast<const float4*>(p.wcur + o);
    v.x += p.l2 * wv.x; v.y += p.l2 * wv.y; v.z += p.l2 * wv.z; v.w += p.l2 * wv.w;
  }
  *reinterpret_cast<float4*>(p.c + o) = v;
}

static const int kTnMaxW = 512;  // 2 workgroups per CU

size_t gemm_tn_ws_bytes(long M, int P, int Q) {
  (void)M; (void)P; (void)Q;
  return (size_t)2 * kTnMaxW * 128 * 128 * sizeof(float);
}

template <int BP, int BQ, bool CONV, int BF>
static hipError_t tn_launch_kernel(const TnDev& d, hipStream_t st) {
  const size_t lds_bytes = BF == 2 ? (size_t)4 * (BP + BQ) * 40 * 2
                                   : (BF ? (size_t)2 * (BP + BQ) * 40 * 2 : (size_t)2 * 32 * (BP + 8 + BQ + 8) * sizeof(float));
  static bool attr_done = false;  // benign race: idempotent attribute
  if (!attr_done) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_tn_f32_mfma<BP, BQ, CONV, BF>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    attr_done = true;
  }
  hipLaunchKernelGGL((gemm_tn_f32_mfma<BP, BQ, CONV, BF>), dim3(d.W), dim3(256), lds_bytes, st, d);
  return hipGetLastError();
}

template <int BP, int BQ>
static hipError_t tn_launch_tile(const TnParams& p, float* ws, hipStream_t st) {
  TnDev d;
  d.p = p;
  d.ws = ws;
  d.msteps = (int)((p.M + 31) / 32);
  d.ptiles = p.P / BP;
  d.qtiles = p.Q / BQ;
  d.units = (long)d.ptiles * d.qtiles * d.msteps;
  d.W = (int)(d.units < kTnMaxW ? d.units : kTnMaxW);
  d.kt = 0;
  // Interleaved row steps for the forms that stage transposed 16-bit operands (bf16, two-term f16), from 18 tiles on:
  // measured at 8 samples (tools/conv_bwd_time.py, r03aa / r03ab) 56 x 56, 256 -> 256: 222 -> 194 us (bf16), 300 -> 275
  // (f16 split); 28 x 28, 256 -> 512: 132 -> 105, 177 -> 153; no gain with 9 tiles (112 x 112) and none for the
  // fp32-MFMA form (MFMA-bound), which keeps the contiguous stream-K ranges.
  const int T = d.ptiles * d.qtiles;
  if (p.bf16 != 0 && T >= 18) {
    int kt = kTnMaxW / T;
    if (kt > d.msteps) kt = d.msteps;
    if (kt < 1) kt = 1;
    if ((long)T * kt <= 2 * kTnMaxW) {
      d.kt = kt;
      d.W = T * kt;
    }
  }
  hipError_t e;
  if (p.Cin > 0)
    e = p.bf16 == 2 ? tn_launch_kernel<BP, BQ, true, 2>(d, st)
                    : (p.bf16 ? tn_launch_kernel<BP, BQ, true, 1>(d, st) : tn_launch_kernel<BP, BQ, true, 0>(d, st));
  else
    e = p.bf16 == 2 ? tn_launch_kernel<BP, BQ, false, 2>(d, st)
                    : (p.bf16 ? tn_launch_kernel<BP, BQ, false, 1>(d, st) : tn_launch_kernel<BP, BQ, false, 0>(d, st));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((tn_fixup<BP, BQ>), dim3(d.ptiles * d.qtiles, BP * BQ / 1024), dim3(256), 0, st, d);
  return hipGetLastError();
}

hipError_t gemm_tn_launch(const TnParams& pin, float* ws, hipStream_t st) {
  TnParams p = pin;
  const bool p128 = p.P % 128 == 0, q128 = p.Q % 128 == 0;
  // the bf16 form pays for its transposing stage only with the 128x128 tile (measured: 64-wide
  // tiles 62 TFLOP/s in bf16 against 76 in fp32)
  if (p.bf16 == 1 && !(p128 && q128)) p.bf16 = 0;
  if (p.bf16 == 2 && (!p.amax_a || !p.amax_b || p.amax_a_n <= 0 || p.amax_b_n <= 0)) p.bf16 = 0;  // no operand maxima: fp32 MFMA
  if (p128 && q128) return tn_launch_tile<128, 128>(p, ws, st);
  if (p128) return tn_launch_tile<128, 64>(p, ws, st);
  if (q128) return tn_launch_tile<64, 128>(p, ws, st);
  return tn_launch_tile<64, 64>(p, ws, st);
}

}  // namespace disn
