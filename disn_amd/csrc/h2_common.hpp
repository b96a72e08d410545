// The building blocks of the two-term f16 split (x = h + l after a power-of-two scale), shared by everything that forms
// or consumes it -- conv_h2.hip, conv_h2w.hip, dense_h2.hip, dense_h2w.hip, mlp_fused.hip, elementwise.hip,
// gemm_tn_mfma.hip (the scale): fragment vector types, the scale, the split itself, the hardware-row <-> logical-row map that makes
// the A-fragment ds_read_b128 conflict-free (see conv_h2.hip), and the pieces the four h2 kernels have in common.
// ONE definition each: two sides of a split operand that disagree on the scale or the rounding disagree in bits.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace disn {

typedef _Float16 ch_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 ch_h4 __attribute__((ext_vector_type(4)));
typedef float ch_f16v __attribute__((ext_vector_type(16)));
typedef float ch_f2v __attribute__((ext_vector_type(2)));

namespace ch2 {
// power of two s with amax * s in [2^target, 2^(target+1)); 1 for amax == 0 / non-finite / extreme
__host__ __device__ inline float pow2_scale(float amax, int target_exp) {
  union { float f; unsigned u; } a;
  a.f = amax;
  const int e = (int)((a.u >> 23) & 0xffu) - 127;
  if (!(amax > 0.f) || e > 100 || e < -100) return 1.0f;
  a.u = (unsigned)(127 + target_exp - e) << 23;
  return a.f;
}
// logical row of hardware row i (0..31) of a 32-row block
__host__ __device__ constexpr int sigma(int i) {
  return i < 4 ? i : (i < 12 ? i + 12 : (i < 16 ? i - 8 : (i < 20 ? i + 8 : (i < 28 ? i - 12 : i))));
}
// first logical row of the four held by accumulator quad q (registers 4q..4q+3) of lane half g
__host__ __device__ constexpr int quad_row(int q, int g) {
  return sigma(8 * q + 4 * g);
}

#ifdef __HIPCC__
// the split of an already scaled value: h = f16(v), l = f16(v - h)
__device__ __forceinline__ void split(float v, _Float16& h, _Float16& l) {
  h = (_Float16)v;
  l = (_Float16)(v - (float)h);
}
// four values, scaled by s, into the h and l planes' quads.  mask (the convolution loaders): ANDed with the bits of every
// value first -- 0 for a unit outside the image, whose load read some valid address
__device__ __forceinline__ void split4(const float (&x)[4], float s, ch_h4& hh, ch_h4& ll, unsigned mask = 0xffffffffu) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    _Float16 h, l;
    split(__uint_as_float(__float_as_uint(x[e]) & mask) * s, h, l);
    hh[e] = h;
    ll[e] = l;
  }
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
// the wave's maximum of vmax (non-negative) -> one atomic maximum into `slot` (bit patterns of non-negative floats order
// as integers).  Producers spread their waves over 64 slots: same-address atomics serialise in L2 (~10 ns each)
__device__ __forceinline__ void publish_wave_max(float vmax, float* slot) {
  vmax = wave_max(vmax);
  if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned*>(slot), __float_as_uint(vmax));
}
// Operand scale of a dense tile (rows m0 .. of problem P; aoff: its image's slot group), first half: this lane's share of
// max |a| (the in_amax / in_amax2 slots) -> amax_lane and of max |in_bias| -> bmax_lane.  The loads are requested where
// this is called; the kernels reduce later, behind their weight queue: sa = pow2_scale(wave_max(amax_lane) +
// wave_max(bmax_lane), 14), since |relu(a + b)| <= max|a| + max|b|.  The bias bound is over the tile's image when the
// maxima are per image (tiles do not straddle images then: the scale must not depend on the batch), else over every
// bias row of the call.
// n1: entries of in_amax (64 slots, or P.in_amax_n where the form takes per-workgroup maxima of a producer).
__device__ __forceinline__ void dense_operand_maxima(const DenseH2Prob& P, int m0, size_t aoff, int lane, int n1,
                                                     float& amax_lane, float& bmax_lane) {
  amax_lane = 0.f;
  for (int i = lane; i < n1; i += 64) amax_lane = fmaxf(amax_lane, P.in_amax[aoff + i]);
  if (P.in_amax2) {
    const int n2 = P.in_amax2_n > 0 ? P.in_amax2_n : 64;
    for (int i = lane; i < n2; i += 64) amax_lane = fmaxf(amax_lane, P.in_amax2[aoff + i]);
  }
  bmax_lane = 0.f;
  if (P.in_bias) {
    const float* ib = P.in_bias;
    int nb = P.in_bias_rows > 0 ? ((P.M + P.in_bias_rows - 1) / P.in_bias_rows) * P.K : P.K;
    if (P.amax_rows > 0 && P.in_bias_rows > 0) { ib += (size_t)(m0 / P.in_bias_rows) * P.K; nb = P.K; }
    for (int i = lane; i < nb; i += 64) bmax_lane = fmaxf(bmax_lane, fabsf(ib[i]));
  }
}
// a finished segment of an MFMA accumulator block -> its fp32 total (register PAIRS, never an MFMA operand).  The segment
// sits in accumulation registers, which VALU cannot read: two v_accvgpr_read + one v_pk_add_f32 per pair, written out so
// that the compiler keeps tot in arch VGPRs instead of shuttling it through the accumulation file around every add
__device__ __forceinline__ void flush_segment(const ch_f16v& acc, ch_f2v (&tot)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    ch_f2v t;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(t[0]) : "a"(acc[2 * r]));
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(t[1]) : "a"(acc[2 * r + 1]));
    asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(tot[r]) : "v"(t));
  }
}
#endif
}  // namespace ch2

// clock stamps of a workgroup (tuning builds; P.stamps == nullptr in the product)
#ifdef DISN_TUNING
#define CH2_STAMP(i) \
  if (P.stamps && threadIdx.x == 0) P.stamps[(size_t)blockIdx.x * 16 + (i)] = (i) == 0 ? (long long)wall_clock64() : (long long)clock64()
#else
#define CH2_STAMP(i)
#endif

// one 3x3 SAME convolution launch of conv_h2.hip / conv_h2w.hip
struct ConvH2Dev {
  const float* in;            // [B][H][W][Cin]
  const unsigned char* wimg;  // conv_h2_pack image
  const float* bias;          // [Cout]
  const float* in_amax;       // 64 floats whose maximum is max |in|
  float* out;                 // [B][H][W][Cout]
  float* pool_out;            // [B][H/2][W/2][Cout] or nullptr
  float* out_amax;            // 64 floats (zeroed by the caller): atomic max |out| spread over the slots, or nullptr
  int B, H, W, Cin, Cout;
  int tiles_x, tiles_y;
  int relu;
  int amax_stride;            // floats between the slot groups of consecutive images (0: one group for the whole batch)
  long long* stamps;  // tuning builds: 16 clock stamps per workgroup (nullptr in the product)
};

// Geometry of every ConvForm (kernels.hpp): what conv_h2_plan() lays a launch out with; conv_h2_go / conv_h2w_go check it
// against the template arguments of the kernel they launch
struct ConvFormGeom {
  int th, tw;    // patch
  int nch;       // output channels per workgroup
  int block;     // threads
  int cin_mult;  // Cin is a multiple of this (whole chunks, whole segments)
  int cin_min;
};
inline constexpr ConvFormGeom kConvForms[CONV_FORMS] = {
    /* CONV_P14_K4 */ {2, 14, 32, 256, 64, 64},
    /* CONV_P14_K8 */ {2, 14, 32, 512, 128, 128},
    /* CONV_P14_K8_OCC2 */ {2, 14, 32, 512, 128, 128},
    /* CONV_P14_K4_OCC2 */ {2, 14, 32, 256, 64, 64},
    /* CONV_P14_K4_OCC2_SEG */ {2, 14, 32, 256, 128, 128},
    /* CONV_IMG14_K4 */ {14, 14, 32, 256, 64, 64},
    /* CONV_IMG14_K4_SEG */ {14, 14, 32, 256, 128, 128},
    /* CONV_P28_N1_K4 */ {2, 28, 32, 256, 64, 64},
    /* CONV_P28_N1_K8 */ {2, 28, 32, 512, 128, 128},
    /* CONV_P28_N2 */ {2, 28, 64, 512, 64, 64},
    /* CONV_P28_N2_OCC2 */ {2, 28, 64, 512, 64, 64},
    /* CONV_P16_N2 */ {8, 16, 64, 512, 64, 64},
    /* CONV_P16H_N2_OCC2 */ {4, 16, 64, 512, 64, 64},
    /* CONVW_P32_N2 */ {8, 32, 64, 256, 16, 16},
    /* CONVW_N4 */ {8, 28, 128, 256, 16, 16},
    /* CONVW_N2 */ {8, 28, 64, 128, 16, 16},
    /* CONVW_N4_K2 */ {8, 28, 128, 512, 32, 32},
    /* CONVW_N2_K2 */ {8, 28, 64, 256, 32, 32},
    // the segmented pair: two K halves of whole two-chunk segments, the second half starting inside the chunk loop
    /* CONVW_N4_PARK */ {8, 28, 128, 256, 64, 128},
    /* CONVW_N2_K2_SEG */ {8, 28, 64, 256, 64, 128},
};

}  // namespace disn
