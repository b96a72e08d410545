"""Shape tables of the training backward kernels' tail cases, and the helpers the training tests share.

Plain module (not a conftest): imported by test_gpu_train_edges.py (which runs every table on the GPU), by
test_train_edges_host.py (which checks on the CPU that the tables still reach the code paths they were chosen for) and,
for the helpers, by test_gpu_train.py / test_gpu_bf16.py.  Every shape is the smallest at which its path runs.
"""
import numpy as np
import torch

from conftest import report_close


# ---- helpers shared by the training tests ---------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def step_feed(B, N, seed):
    """a synthetic feed of the whole step: B images, N points each, their rotated copies and sdf values"""
    from oracle import disn_oracle as O
    feed = O.synth_inputs(seed=seed, batch=B, n_points=N)
    rng = np.random.default_rng(seed + 1)
    feed["sample_pc_rot"] = (feed["sample_pc"] @ np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32)).astype(np.float32)
    feed["sdf"] = (0.05 * rng.standard_normal((B, N, 1))).astype(np.float32)
    return feed


def rel_close(name, got, ref, rtol_of_max):
    ref = np.asarray(ref, np.float64)
    report_close(name, got, ref, atol=rtol_of_max * max(float(np.abs(ref).max()), 1e-30))


# ---- disn_conv3x3_backward: (B, H, W, Cin, Cout) ----------------------------------------------------------------------
MODES = (0, 1, 2)                      # compute_bf16: f32-input MFMA, bf16 multiply, fp32-accurate two-term f16
CONV_SHAPES = [
    (1, 1, 1, 64, 64),       # M = 1: every tap but the centre outside; 64x64 tile, 9 units
    (1, 1, 7, 128, 64),      # one-row image, M = 7; 128x64 tile (also in mode 2)
    (1, 7, 1, 64, 128),      # one-column image; 64x128 tile
    (3, 5, 7, 64, 128),      # odd W, odd M = 105: row pairs straddle image rows and images
    (1, 7, 5, 128, 128),     # M = 35 = 32 + 3; 128x128 tile, T = 9: contiguous stream-K in every mode
    (3, 3, 3, 128, 256),     # M = 27 < 32; T = 18: interleaved in modes 1 and 2, kt clamped to msteps = 1
    (5, 9, 11, 128, 256),    # M = 495, msteps = 16, kt 28 -> 16; B >= 4: the batched data gradient
    (4, 13, 6, 192, 192),    # 64x64 tile, T = 81: mode 2 interleaved with kt = 6, mode 1 falls back to fp32; B at the switch
    (3, 13, 6, 192, 192),    # ... one sample below the switch
    (2, 33, 31, 64, 64),     # units = 576 > 512: contiguous segments cross tile boundaries, slabs + fix-up
    (1, 2, 2, 512, 512),     # M = 4 with T = 144
]
CONV_C3_SHAPES = [(1, 1, 1, 3, 64), (3, 5, 7, 3, 64), (2, 33, 31, 3, 64)]   # the Cin = 3 im2col path, need_dx = False
CONV_ZERO_SHAPE = (3, 5, 7, 64, 128)   # the all-zero / one-sample-zero dy cases
CONV_WD = 1e-3
CONV_BATCHED_FROM = 4                  # kConvWideMinImages (kernels.hpp): images from which the data gradient is batched

# ---- disn_dense_backward: (M, K, N) -----------------------------------------------------------------------------------
DENSE_SHAPES = [
    (1, 64, 64),
    (31, 64, 128),
    (33, 128, 64),
    (95, 192, 192),
    (65, 128, 256),          # odd M on the 128x128 bf16 tile
    (64, 4096, 4096),        # T = 1024: interleaved with kt = 1 and W = 1024, every slab in use
    (65, 4096, 4224),        # T = 1056 > 1024: back to the contiguous split
]
DENSE_WD = 1e-3

# ---- disn_maxpool2x2_backward: (B, H, W, C) ---------------------------------------------------------------------------
POOL_SHAPES = [(1, 2, 2, 4), (3, 6, 10, 8), (2, 14, 2, 64), (1, 2, 30, 12)]
POOL_CONTINUOUS_SHAPE = (3, 6, 10, 8)

# ---- disn_resize_bilinear_backward: (B, Hin, Win, C, cs, coff, Hout, Wout) --------------------------------------------
RESIZE_SHAPES = [
    (1, 1, 1, 4, 4, 0, 137, 137),
    (2, 68, 68, 4, 8, 4, 137, 137),      # separable, exactly at the threshold (137 >= 2 * 68)
    (2, 69, 69, 4, 4, 0, 137, 137),      # the first non-separable size
    (3, 68, 69, 8, 16, 8, 137, 137),     # the two axes on opposite sides of the threshold
    (3, 69, 14, 8, 8, 0, 137, 137),
    (1, 137, 137, 4, 4, 0, 137, 137),    # identity: dout's slice bit for bit
    (2, 14, 28, 4, 4, 0, 137, 137),
    (1, 224, 112, 4, 4, 0, 137, 137),
    (1, 7, 3, 4, 4, 0, 10, 9),           # an output that is not 137
]

# ---- disn_gather_backward (B, N), disn_adam_update n, disn_train_step (B, N) ------------------------------------------
GATHER_SHAPES = [(1, 1), (3, 257), (1, 64)]
ADAM_SIZES = [4, 1020, 1024, 1028, (1 << 22) + 4]
ADAM_GRAD_SCALES = [1.0, 0.5]
STEP_SHAPES = [(1, 100), (3, 37)]
STEP_PRECISIONS = ["f32", "f32_mfma"]


# ---- what the two entries hand to gemm_tn_launch (train.hip: conv_bwd, dense_bwd) ------------------------------------
def conv_tn_problem(shape, mode):
    """-> (M, P, Q, requested mode, implicit im2col) of the weight-gradient GEMM of a disn_conv3x3_backward call"""
    B, H, W, Cin, Cout = shape
    if Cin == 3:                       # explicit 64-column im2col, always on the f32-input MFMA
        return B * H * W, 64, Cout, 0, False
    return B * H * W, 9 * Cin, Cout, mode, True


def dense_tn_problem(shape, mode):
    """... of a disn_dense_backward call: the two-term f16 form needs operand maxima, which only the convolution has"""
    M, K, N = shape
    return M, K, N, 1 if mode == 1 else 0, False
