// One training batch out of the device-resident training set (disn_amd/data_resident.py): the feed of
// disn_train_step -- imgs, sample_pc, sample_pc_rot, sdf, trans_mat -- from three small index arrays, one launch.
// THIS FILE IS COMPILED WITH -ffp-contract=off: every output is compared bit for bit with the host loader
// (data_sdf.Pt_sdf_img.get_batch followed by train_sdf.feed_from_batch), sample_pc_rot within the rounding of a
// three-term fp32 dot product.  DESIGN §4t.
//
//   imgs[b]          = clip(rgb, 0, 255) / 255 of img[view_idx[b]] (uint8 RGBA: the clip is the identity), one IEEE
//                      division per channel; with backcolorwhite, alpha == 0 -> 255 / 255
//   sample_pc[b, s]  = samples[sample_off[obj] + choice[b, s]].xyz         obj = obj_idx[b], one 16-byte load per row
//   sdf[b, s]        = that row's w - 0.003f                               (train/train_sdf.py:375)
//   sample_pc_rot    = sample_pc, or with rot: column j = (p0*R[0][j] + p1*R[1][j]) + p2*R[2][j], R = obj_rot_mat[view]
//   trans_mat[b]     = trans_mat_all[view_idx[b]]
//
// Grid (point blocks + pixel blocks, B): blockIdx.y is the sample, so obj, view, the row range and R are the same
// for every lane of a block (scalar loads); blockIdx.x < pt_blocks takes 256 points, the others 256 pixels each.
// An index outside its range (obj, view, or a choice outside the object's rows) reads nothing: the outputs it
// would have produced are 0 and flags[0] is set to 1 (every writer stores the same value: no atomics).
#include "../../include/disn_amd.h"
#include "kernels.hpp"

namespace disn {

namespace {

constexpr int kPixels = DISN_IMG_H * DISN_IMG_W;

struct AssembleArgs {
  const float4* samples;
  const int64_t* sample_off;
  int64_t n_obj;
  const uchar4* img;
  const float* trans_mat_all;
  const float* rot_all;
  int64_t n_view;
  const int* obj_idx;
  const int* view_idx;
  const int* choice;
  int S, pt_blocks, rot, white;
  float* imgs;
  float* sample_pc;
  float* sample_pc_rot;
  float* sdf;
  float* trans_mat;
  int* flags;
};

__global__ void __launch_bounds__(256) assemble_batch_kernel(const AssembleArgs a) {
  const int b = blockIdx.y;
  const int64_t obj = a.obj_idx[b], view = a.view_idx[b];
  const bool view_ok = view >= 0 && view < a.n_view;
  if ((int)blockIdx.x < a.pt_blocks) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 12)
      a.trans_mat[b * 12 + threadIdx.x] = view_ok ? a.trans_mat_all[view * 12 + threadIdx.x] : 0.f;
    if (s >= a.S) return;
    int64_t off = 0, cnt = 0;
    if (obj >= 0 && obj < a.n_obj) {
      off = a.sample_off[obj];
      cnt = a.sample_off[obj + 1] - off;
    }
    const int64_t o = (int64_t)b * a.S + s;
    const int c = a.choice[o];
    float4 p = make_float4(0.f, 0.f, 0.f, 0.003f);
    const bool ok = c >= 0 && c < cnt && (view_ok || !a.rot);
    if (ok) p = a.samples[off + c];
    else a.flags[0] = 1;
    a.sample_pc[3 * o] = p.x;
    a.sample_pc[3 * o + 1] = p.y;
    a.sample_pc[3 * o + 2] = p.z;
    a.sdf[o] = p.w - 0.003f;
    if (a.rot && ok) {
      const float* R = a.rot_all + view * 9;
      a.sample_pc_rot[3 * o] = (p.x * R[0] + p.y * R[3]) + p.z * R[6];
      a.sample_pc_rot[3 * o + 1] = (p.x * R[1] + p.y * R[4]) + p.z * R[7];
      a.sample_pc_rot[3 * o + 2] = (p.x * R[2] + p.y * R[5]) + p.z * R[8];
    } else {
      a.sample_pc_rot[3 * o] = p.x;
      a.sample_pc_rot[3 * o + 1] = p.y;
      a.sample_pc_rot[3 * o + 2] = p.z;
    }
    return;
  }
  const int px = ((int)blockIdx.x - a.pt_blocks) * 256 + threadIdx.x;
  if (px >= kPixels) return;
  float r = 0.f, g = 0.f, bl = 0.f;
  if (view_ok) {
    const uchar4 q = a.img[view * kPixels + px];
    const bool bg = a.white && q.w == 0;
    r = bg ? 255.f : (float)q.x;
    g = bg ? 255.f : (float)q.y;
    bl = bg ? 255.f : (float)q.z;
  } else {
    a.flags[0] = 1;
  }
  float* out = a.imgs + ((int64_t)b * kPixels + px) * 3;
  out[0] = __fdiv_rn(r, 255.f);
  out[1] = __fdiv_rn(g, 255.f);
  out[2] = __fdiv_rn(bl, 255.f);
}

}  // namespace

static hipError_t assemble_batch_launch(const float* samples, const int64_t* sample_off, int64_t n_obj,
                                        const unsigned char* img, const float* trans_mat_all, const float* rot_all,
                                        int64_t n_view, const int* obj_idx, const int* view_idx, const int* choice,
                                        int B, int S, int rot, int white, float* imgs, float* sample_pc,
                                        float* sample_pc_rot, float* sdf, float* trans_mat, int* flags,
                                        hipStream_t st) {
  AssembleArgs a;
  a.samples = reinterpret_cast<const float4*>(samples);
  a.sample_off = sample_off;
  a.n_obj = n_obj;
  a.img = reinterpret_cast<const uchar4*>(img);
  a.trans_mat_all = trans_mat_all;
  a.rot_all = rot_all;
  a.n_view = n_view;
  a.obj_idx = obj_idx;
  a.view_idx = view_idx;
  a.choice = choice;
  a.S = S;
  a.pt_blocks = (S + 255) / 256;
  a.rot = rot;
  a.white = white;
  a.imgs = imgs;
  a.sample_pc = sample_pc;
  a.sample_pc_rot = sample_pc_rot;
  a.sdf = sdf;
  a.trans_mat = trans_mat;
  a.flags = flags;
  const unsigned gx = (unsigned)a.pt_blocks + (unsigned)((kPixels + 255) / 256);
  assemble_batch_kernel<<<dim3(gx, (unsigned)B), 256, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace disn

// ---- the C entries of include/disn_amd.h: argument and workspace checks, then the launchers above ----
using namespace disn;

#define DISN_TRY(expr)                    \
  do {                                    \
    hipError_t _e = (expr);               \
    if (_e != hipSuccess) return (int)_e; \
  } while (0)

extern "C" {

int disn_assemble_batch(const float* samples, const int64_t* sample_off, int64_t n_obj, const uint8_t* img,
                        const float* trans_mat_all, const float* rot_all, int64_t n_view, const int32_t* obj_idx,
                        const int32_t* view_idx, const int32_t* choice, int B, int S, int rot, int backcolorwhite,
                        float* imgs, float* sample_pc, float* sample_pc_rot, float* sdf, float* trans_mat,
                        int32_t* flags, void* stream) {
  if (!samples || !sample_off || !img || !trans_mat_all || !obj_idx || !view_idx || !choice || !imgs || !sample_pc ||
      !sample_pc_rot || !sdf || !trans_mat || !flags || (rot && !rot_all) || n_obj < 1 || n_view < 1 || B < 1 || S < 1)
    return DISN_E_ARG;
  if (((uintptr_t)samples & 15) || ((uintptr_t)img & 3)) return DISN_E_ARG;   // float4 rows, uchar4 pixels
  if (B > 65535 || !disn::fits_int(B, S, 3)) return DISN_E_SHAPE;
  if (!disn::fits_int(n_obj, 2) || !disn::fits_int(n_view, 2)) return DISN_E_SHAPE;   // obj_idx / view_idx are int32
  DISN_TRY(assemble_batch_launch(samples, sample_off, n_obj, img, trans_mat_all, rot_all, n_view, obj_idx, view_idx,
                                 choice, B, S, rot != 0, backcolorwhite != 0, imgs, sample_pc, sample_pc_rot, sdf,
                                 trans_mat, flags, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
