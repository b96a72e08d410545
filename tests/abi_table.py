"""One table of the C ABI (include/*.h): every prototype parsed from the headers, checked against the ctypes binding
(disn_amd/_lib.py), and for every entry one CASE -- the smallest legal call -- from which the argument sweep
(tests/test_abi_errors_host.py) and the sanitizer program (tools/abi_sanitize.py) derive their mutated calls.

A CASE never runs as it stands: only its mutations do, each of which the entry must refuse on the host, before anything
is enqueued.  Device pointers are therefore a fake non-null address (FAKE) that no host path may dereference; host
pointers (names ending in _host, struct pointers, paths, boxes, out-parameters) get real memory.

The calls are plain data (Call tuples of argument tokens), so that the same list can be issued through ctypes or written
out as literal C++ calls:
    int / float                a literal
    ("null",) ("fake",)        a NULL / the fake device pointer
    ("host", code, values)     a host array (struct-module type code: f d i q Q B)
    ("obj", kind)              a host object: vgg mlp cam eq layout cam_layout taps5 box6 k9 slot path
    ("need", query, args, d)   query(*args) + d bytes, evaluated when the call is made
    ("big",)                   2^62 bytes: a workspace size that can never be the reason for a refusal
"""
from __future__ import annotations

import glob
import os
import re
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX, INT64_MAX = 2 ** 31 - 1, 2 ** 63 - 1
FAKE = 0x10000                      # non-null, 64 KiB aligned, never mapped: a host dereference is a crash, not a pass
E_ARG, E_SHAPE, E_WS = -1, -2, -3

Proto = namedtuple("Proto", "ret name params header")      # params: [(C type, name)]
# expect: ("eq", v) ("neg",) ("zero",) ("pos",) ("zero_or_ge", token: the CASE's own value); ("eq_if_need", v) and
# ("neg_if_need", token) are made only where the CASE's workspace query gives > 0
Call = namedtuple("Call", "entry label args expect")


# ---------------------------------------------------------------- the headers ------------------------------------
def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def header_paths():
    return sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))


def parse_param(p):
    p = " ".join(p.split())
    m = re.match(r"^(.*?)(\w+)\s*(\[\d*\])?$", p)
    assert m and m.group(1).strip(), "cannot parse parameter %r" % p
    ctype = m.group(1).strip().replace(" *", "*")
    if m.group(3):
        ctype += "*"                                   # an array parameter is a pointer
    return ctype, m.group(2)


def parse_headers():
    """name -> Proto of every function declared in include/*.h"""
    out = {}
    for path in header_paths():
        text = strip_comments(open(path).read())
        text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
        for ret, name, params in re.findall(r"([\w\s\*]+?)\b(disn_\w+)\s*\(([^)]*)\)\s*;", text):
            assert name not in out, "%s declared twice" % name
            params = params.strip()
            plist = [] if params in ("", "void") else [parse_param(p) for p in params.split(",")]
            out[name] = Proto(" ".join(ret.split()), name, plist, os.path.basename(path))
    return out


def c_class(ctype):
    """pointer / int / int64_t / size_t / float / double / uint32_t"""
    if "*" in ctype:
        return "pointer"
    t = ctype.replace("const ", "").strip()
    assert t in ("int", "int64_t", "size_t", "float", "double", "uint32_t"), ctype
    return t


def binding_class(t):
    import ctypes as C
    if t in (C.c_void_p, C.c_char_p) or isinstance(t, type(C.POINTER(C.c_int))):
        return "pointer"
    return {C.c_int: "int", C.c_int64: "int64_t", C.c_size_t: "size_t", C.c_float: "float", C.c_double: "double",
            C.c_uint32: "uint32_t"}[t]


def binding_tables():
    from disn_amd import _lib
    return (_lib.SIGNATURES, _lib.SIGNATURES_SIMPLIFY, _lib.SIGNATURES_COLOUR, _lib.SIGNATURES_SAMPLE,
            _lib.SIGNATURES_SMOOTH)


def binding():
    out = {}
    for t in binding_tables():
        assert not set(t) & set(out)
        out.update(t)
    return out


def check_against_binding(protos=None):
    """the parsed headers and the five signature tables describe the same functions: name, arity, class of every
    parameter and of the return value"""
    protos = protos or parse_headers()
    sig = binding()
    assert set(protos) == set(sig), sorted(set(protos) ^ set(sig))
    for name, p in protos.items():
        res, args = sig[name]
        assert c_class(p.ret) == binding_class(res), (name, p.ret, res)
        assert len(p.params) == len(args), (name, len(p.params), len(args))
        for (ctype, pname), a in zip(p.params, args):
            assert c_class(ctype) == binding_class(a), (name, pname, ctype, a)


# ---------------------------------------------------------------- the cases --------------------------------------
def _kv(s):
    out = {}
    for item in s.split():
        k, v = item.split("=")
        out[k] = float(v) if ("." in v or "e" in v) else int(v)
    return out


class Case:
    def __init__(self, sizes, flags, need, host, nullable, zero_ok, no_extreme, required, positive):
        self.sizes, self.flags, self.need, self.host = _kv(sizes), _kv(flags), need, host
        self.nullable, self.zero_ok, self.no_extreme = nullable, zero_ok, no_extreme
        self.required, self.positive = required, positive


def E(sizes="", flags="", need=None, host=None, nullable=None, zero_ok=None, no_extreme=None, required=()):
    """an entry that returns a status.
    sizes       the counts and sizes (mutated to 0, -1 and the type's maximum), `name=value ...`
    flags       every other scalar (modes, offsets, capacities, floats other than 1.0): never mutated
    need        size_t parameter -> (the pointer it sizes, "query(args)"): args are expressions over the sizes
    host        pointer -> (type code, values): host memory the entry reads or writes
    nullable    pointer -> the header's own words for why it may be NULL (the CASE passes NULL there)
    zero_ok     size -> the status of 0 where the header gives 0 a meaning; None: 0 is legal and reaches the device,
                so it is not called
    no_extreme  size -> why the type's maximum cannot be passed (a host buffer of that length is the caller's promise)
    required    `stream` is NULL-able everywhere but in the entries that list it here"""
    return Case(sizes, flags, need or {}, host or {}, nullable or {}, zero_ok or {}, no_extreme or {}, required, True)


def Q(sizes="", flags="", positive=True, zero_ok=()):
    """a size query: a non-positive size gives 0; `positive`: the CASE's own arguments give > 0; zero_ok: the sizes for
    which 0 is a legal value (an empty mesh) and only a negative one gives 0"""
    return Case(sizes, flags, {}, {}, {}, {k: None for k in zero_ok}, {}, (), positive)


# entries without arguments to mutate, or whose return value is not a status
NO_MUTATION = {
    "disn_abi_version": "no arguments",
    "disn_conv1_1_workspace_bytes": "no arguments",
    "disn_fold_local_workspace_bytes": "no arguments",
    "disn_mlp_fused_image_bytes": "no arguments",
    "disn_mlp_fused_feat_image_bytes": "no arguments",
    "disn_crc32c": "returns a checksum, not a status: any (pointer, length) is the caller's promise",
}

VOFF, FOFF = ("q", [0, 3]), ("q", [0, 1])                  # one mesh: three vertices, one triangle
TRI_V, TRI_F = ("f", [0, 0, 0, 1, 0, 0, 0, 1, 0]), ("i", [0, 1, 2])
MESH_HOST = {"v_off_host": VOFF, "f_off_host": FOFF}
MESH_B = {"B": "v_off_host / f_off_host hold B + 1 entries, which the entry reads"}
RESIZED = "resized224 may be NULL: the resized images then stay inside ws"
MESH_Q = ("nv_total", "nf_total")                          # an empty mesh is legal
CONV = "B=1 H=8 W=8 Cin=32 Cout=64"
CONV_SPLITK = "B=1 H=2 W=2 Cin=512 Cout=64"              # the f32 GEMM splits K here, hence takes a workspace
CONV64 = "B=1 H=8 W=8 Cin=64 Cout=64"
GRID = dict(sizes="R=4 k1=125", flags="k0=0")


def _ws(q):
    return {"ws_bytes": ("ws", q)}


CASES = {
    # ---- include/disn_amd.h
    "disn_pack_kn": E("K=32 N=64 Kpad=32"),
    "disn_pack_kn_x3_bytes": Q("K=32 N=64"),
    "disn_pack_kn_x3": E("K=32 N=64"),
    "disn_conv3x3_x3_workspace_bytes": Q(CONV),
    "disn_conv3x3_x3": E(CONV, "relu=1", _ws("disn_conv3x3_x3_workspace_bytes(B,H,W,Cin,Cout)")),
    "disn_pack_conv_h2_bytes": Q("Cin=64 Cout=64"),
    "disn_pack_conv_h2": E("Cin=64 Cout=64"),
    "disn_conv_h2_gain_span": E("Cin=64 Cout=64", host={"span_log2": ("f", [0])}),
    "disn_conv1_1": E("B=1 H=8 W=8", "relu=1", _ws("disn_conv1_1_workspace_bytes()"),
                      nullable={"out_amax": "optional out_amax = max |out|"}),
    "disn_conv3x3_h2_workspace_bytes": Q("B=1"),
    "disn_conv3x3_h2": E(CONV64, "relu=1 tiling=0", _ws("disn_conv3x3_h2_workspace_bytes(B)"),
                         nullable={"pool_out": "optional pool_out", "out_amax": "optional out_amax"}),
    "disn_conv3x3_h2_plan": E(CONV64, "tiling=0", host={"grid": ("i", [0]), "block": ("i", [0])},
                              nullable={"grid": "either may be NULL", "block": "either may be NULL"}),
    "disn_resize_bilinear": E("B=1 Hin=2 Win=2 C=3 Hout=4 Wout=4 out_cstride=3", "out_coff=0"),
    "disn_vgg16_workspace_bytes": Q("B=1"),
    "disn_vgg16_forward": E("B=1", need=_ws("disn_vgg16_workspace_bytes(B)"), nullable={"resized224": RESIZED}),
    "disn_vgg16_conv_stack": E("B=1", need=_ws("disn_vgg16_workspace_bytes(B)"),
                               nullable={"pool5": "pool5 [B,7,7,512] optional (NULL: not copied out)",
                                         "resized224": RESIZED}),
    "disn_conv3x3_workspace_bytes": Q(CONV_SPLITK),
    "disn_conv3x3": E(CONV_SPLITK, "relu=1", _ws("disn_conv3x3_workspace_bytes(B,H,W,Cin,Cout)")),
    "disn_conv3x3_planned_workspace_bytes": Q(CONV, "bm=64 bn=64 wgs=2"),
    "disn_conv3x3_planned": E(CONV, "relu=1 bm=64 bn=64 wgs=2",
                              _ws("disn_conv3x3_planned_workspace_bytes(B,H,W,Cin,Cout,64,64,2)")),
    "disn_maxpool2x2": E("B=1 H=2 W=2 C=64"),
    "disn_fc_workspace_bytes": Q("B=1 K=64 N=256"),
    "disn_fc": E("B=1 K=64 N=256", "relu=1", _ws("disn_fc_workspace_bytes(B,K,N)")),
    "disn_pack_dense_h2_bytes": Q("K=64 N=64"),
    "disn_pack_dense_h2": E("K=64 N=64"),
    "disn_dense_h2_workspace_bytes": Q("images=1"),
    "disn_dense_h2": E("lda1=64 k1=64 M=64 N=64", "lda2=0 k2=0 rows_per_image=0 image_k=0 k_begin=0 relu=1",
                       _ws("disn_dense_h2_workspace_bytes(1)"),
                       nullable={"a2": "k2 may be 0 with a2 NULL", "in_bias": "the identity when in_bias is NULL",
                                 "add_in": "add_in != NULL = a partial product formed earlier",
                                 "out_amax": "Optional out_amax"}),
    "disn_get_loss": E("M=4"),
    "disn_fc_t": E("B=1 K=64 N=64", "relu=1"),
    "disn_dense_workspace_bytes": Q("M=8 K=512 N=64"),          # the smallest shape that splits K, hence takes a workspace
    "disn_dense": E("lda1=512 k1=512 M=8 N=64", "lda2=0 k2=0 relu=1", _ws("disn_dense_workspace_bytes(M,k1,N)"),
                    nullable={"a2": "k2 may be 0 with a2 NULL"}),
    "disn_build_featmap": E("B=1"),
    "disn_project": E("B=1 N=4"),
    "disn_gather": E("B=1 N=4"),
    "disn_gather_taps": E("B=1 N=4"),
    "disn_gather_taps_split": E("B=1 N=128"),
    "disn_gather_fold": E("N=4"),
    "disn_mlp_fused_pack": E(),
    "disn_mlp_fused_feat_pack": E(),
    "disn_query_taps_fused_workspace_bytes": Q("B=1 N=128"),
    "disn_query_taps_fused": E("B=1 N=128", need=_ws("disn_query_taps_fused_workspace_bytes(B,N)")),
    "disn_amax": E("n=4"),
    "disn_query_fused_workspace_bytes": Q("B=1 N=128"),
    "disn_query_fused": E("B=1 N=128", need=_ws("disn_query_fused_workspace_bytes(B,N)")),
    "disn_query_grid_fused_workspace_bytes": Q("max_points=125"),
    "disn_query_grid_fused": E(need=_ws("disn_query_grid_fused_workspace_bytes(k1)"), **GRID),
    "disn_query_grid_listed_workspace_bytes": Q("max_points=8"),
    "disn_query_grid_listed": E("R=4 n=8", "stride=2 first=0", _ws("disn_query_grid_listed_workspace_bytes(n)"),
                                nullable={"idx": "with idx = NULL points first .. first + n - 1 of the lattice"},
                                zero_ok={"n": 0}),
    "disn_grid_band_select_workspace_bytes": Q("R=4", "stride=2"),
    "disn_grid_band_select": E("R=4", "stride=2 dilate=1 idx_capacity=98 iso=0.0 margin=0.5",
                               _ws("disn_grid_band_select_workspace_bytes(R,2)")),
    "disn_grid_band_fill": E("R=4", "stride=2"),
    "disn_sdf_mlp_workspace_bytes": Q("B=1 N=8"),
    "disn_sdf_mlp": E("B=1 N=8", need=_ws("disn_sdf_mlp_workspace_bytes(B,N)"),
                      nullable={"sdf_global": "sdf_global / sdf_local optional (NULL ok)",
                                "sdf_local": "sdf_global / sdf_local optional (NULL ok)"}),
    "disn_query_workspace_bytes": Q("B=1 N=8"),
    "disn_query": E("B=1 N=8", need=_ws("disn_query_workspace_bytes(B,N)")),
    "disn_stream_create": E(required=("stream",)),
    "disn_stream_destroy": E(required=("stream",)),
    "disn_ctx_create": E(),
    "disn_ctx_destroy": E(),
    "disn_ctx_pipeline": E(nullable={"wait_event": "NULL: at once", "record_event": "NULL: nothing"}),
    "disn_encode_workspace_bytes": Q("B=1"),
    "disn_encode": E("B=1", need=_ws("disn_encode_workspace_bytes(B)"),
                     nullable={"ctx": "accepts a context for symmetry and ignores it (may be NULL)",
                               "resized224": RESIZED}),
    "disn_encode_query_workspace_bytes": Q("B=1 N=8"),
    "disn_encode_query": E("B=1 N=8", need=_ws("disn_encode_query_workspace_bytes(B,N)"),
                           nullable={"featmap": "featmap may be NULL: the map is never materialised",
                                     "resized224": RESIZED}),
    "disn_query_grid_ctx_workspace_bytes": Q("max_points=125"),
    "disn_query_grid_ctx": E(need=_ws("disn_query_grid_ctx_workspace_bytes(k1)"), **GRID),
    "disn_equalise_weights": E(host={"tap_scale_host": ("f", [0] * 1472), "span_log2_host": ("f", [0] * 23)},
                               nullable={"span_log2_host": "span_log2 (optional, 23 floats)"}),
    "disn_scale_channels": E("rows=1 C=64", "invert=0", zero_ok={"rows": 0}),
    "disn_dense_bf16_workspace_bytes": Q("M=64 K=32 N=64"),
    "disn_dense_bf16": E("lda1=32 k1=32 M=64 N=64", "lda2=0 k2=0 relu=1 nsplit=1",
                         _ws("disn_dense_bf16_workspace_bytes(M,k1,N)"), nullable={"a2": "k2 may be 0 with a2 NULL"}),
    "disn_conv3x3_bf16_workspace_bytes": Q(CONV),
    "disn_conv3x3_bf16": E(CONV, "relu=1 nsplit=1", _ws("disn_conv3x3_bf16_workspace_bytes(B,H,W,Cin,Cout)")),
    "disn_cam_head": E("B=1", nullable={"K_host": "NULL = the reference's constant"}),
    "disn_param_layout": E(),
    "disn_cam_param_layout": E(),
    "disn_cam_train_workspace_bytes": Q("B=1 N=8"),
    "disn_cam_train_step": E("B=1 N=8", "loss_mode=0 compute_bf16=0", _ws("disn_cam_train_workspace_bytes(B,N)"),
                             nullable={"ctx": "ctx (may be NULL)", "K_host": "9 floats in HOST memory or NULL"}),
    "disn_cam_loss_backward_workspace_bytes": Q("B=1 N=8"),
    "disn_cam_loss_backward": E("B=1 N=8", "loss_mode=0", _ws("disn_cam_loss_backward_workspace_bytes(B,N)"),
                                nullable={"K_host": "9 floats in HOST memory or NULL"}),
    "disn_train_workspace_bytes": Q("B=1 N=64"),
    "disn_train_step": E("B=1 N=64", "compute_bf16=0", _ws("disn_train_workspace_bytes(B,N)"),
                         nullable={"ctx": "ctx (may be NULL)", "head_ready_event": "head_ready_event (may be NULL)"}),
    "disn_adam_update": E("n=4"),
    "disn_dense_backward_workspace_bytes": Q("M=64 K=64 N=64"),
    "disn_dense_backward": E("lda=64 K=64 M=64 N=64", "compute_bf16=0", _ws("disn_dense_backward_workspace_bytes(M,K,N)"),
                             nullable={"y": "with y non-NULL it is masked in place", "da": "da [M][K] (NULL: skipped)"}),
    "disn_conv3x3_backward_workspace_bytes": Q(CONV64),
    "disn_conv3x3_backward": E(CONV64, "compute_bf16=0", _ws("disn_conv3x3_backward_workspace_bytes(B,H,W,Cin,Cout)"),
                               nullable={"y": "with y non-NULL it is masked in place",
                                         "dx": "Cin == 3 (dx must be NULL)"}),
    "disn_maxpool2x2_backward": E("B=1 H=2 W=2 C=64"),
    "disn_resize_bilinear_backward_workspace_bytes": Q("B=1 Hin=2 Win=2 C=4 Hout=4 Wout=4"),
    "disn_resize_bilinear_backward": E("B=1 Hin=2 Win=2 C=4 Hout=4 Wout=4 out_cstride=4", "out_coff=0 accumulate=0",
                                       _ws("disn_resize_bilinear_backward_workspace_bytes(B,Hin,Win,C,Hout,Wout)")),
    "disn_gather_backward": E("B=1 N=4"),
    "disn_mc_workspace_bytes": Q("R=4"),
    "disn_mc_count": E("R=4", "iso=0.0", _ws("disn_mc_workspace_bytes(R)")),
    "disn_mc_emit": E("R=4", "iso=0.0", _ws("disn_mc_workspace_bytes(R)")),
    "disn_mc_batch_workspace_bytes": Q("B=1 R=4"),
    "disn_mc_count_batch": E("B=1 R=4", "iso=0.0", _ws("disn_mc_batch_workspace_bytes(B,R)")),
    "disn_mc_emit_batch": E("B=1 R=4", "iso=0.0", _ws("disn_mc_batch_workspace_bytes(B,R)"),
                            host={"sdf_params_host": ("d", [-1, -1, -1, 1, 1, 1])},
                            no_extreme={"B": "sdf_params_host holds B boxes, which the entry reads"}),
    "disn_write_obj": E("nv=3 nf=1", host={"verts_host": TRI_V, "faces_host": TRI_F}, zero_ok={"nv": 0, "nf": 0},
                        no_extreme={"nv": "verts_host holds nv rows", "nf": "faces_host holds nf rows"}),
    "disn_write_obj_normals": E("nv=3 nf=1", host={"verts_host": TRI_V, "normals_host": TRI_V, "faces_host": TRI_F},
                                zero_ok={"nv": 0, "nf": 0},
                                no_extreme={"nv": "verts_host holds nv rows", "nf": "faces_host holds nf rows"}),
    "disn_read_obj_verts": E(flags="cap=3", host={"verts_host": TRI_V},
                             nullable={"verts_host": "NULL / cap 0: count only"}),
    "disn_read_obj_mesh": E(flags="vcap=3 fcap=1", host={"verts_host": TRI_V, "faces_host": TRI_F, "counts": ("q", [0, 0])},
                            nullable={"verts_host": "NULL / 0: count only", "faces_host": "NULL / 0: count only"}),
    "disn_mesh_bvh_bytes": Q("nf=1"),
    "disn_mesh_bvh_build": E("nv=3 nf=1", need={"bvh_bytes": ("bvh_host", "disn_mesh_bvh_bytes(nf)")},
                             host={"verts_host": TRI_V, "faces_host": TRI_F, "bvh_host": ("B", [0] * 4096)},
                             no_extreme={"nf": "faces_host holds nf rows"}),
    "disn_mesh_udf_points": E("nf=1 n=4", "brute=0"),
    "disn_mesh_udf_grid": E("nf=1 nx=2 ny=2 nz=2", "brute=0"),
    "disn_mesh_sign_workspace_bytes": Q("nx=2 ny=2 nz=2"),
    "disn_mesh_sign": E("nf=1 nx=2 ny=2 nz=2", "steps=1", _ws("disn_mesh_sign_workspace_bytes(nx,ny,nz)"),
                        nullable={"outside": "outside [N] uint8 optional (NULL)"}),
    "disn_mesh_bvh_build_order": E("nv=3 nf=1", need={"bvh_bytes": ("bvh_host", "disn_mesh_bvh_bytes(nf)")},
                                   host={"verts_host": TRI_V, "faces_host": TRI_F, "bvh_host": ("B", [0] * 4096),
                                         "order_host": ("i", [0])},
                                   nullable={"order_host": "order_host NULL: disn_mesh_bvh_build"},
                                   no_extreme={"nf": "faces_host holds nf rows"}),
    "disn_render_views": E("nf=1 V=1 H=2 W=2 S=1", "ambient=0.5 brute=0",
                           nullable={"albedo": "NULL = 0.8 grey", "order": "order is required with albedo or face", "depth": "depth [V,H,W] f32 (optional)",
                                     "face": "face [V,H,W] i32 (optional)"}),
    "disn_trace_state_bytes": Q("n_rays=4"),
    "disn_trace_setup": E("V=1 H=2 W=2", "t_min=0.0", {"state_bytes": ("state", "disn_trace_state_bytes(V*H*W)")}),
    "disn_trace_advance": E("V=1 H=2 W=2 n_active=4", "max_steps=8 list_in=0 refine=2 iso=0.0 eps=0.001 min_step=0.001",
                            {"state_bytes": ("state", "disn_trace_state_bytes(V*H*W)")}),
    "disn_trace_collect": E("V=1 H=2 W=2", need={"state_bytes": ("state", "disn_trace_state_bytes(V*H*W)")}),
    "disn_trace_shade": E("V=1 H=2 W=2 n_hits=1", "iso=0.0 ambient=0.5",
                          {"state_bytes": ("state", "disn_trace_state_bytes(V*H*W)")},
                          nullable={k: "Each output may be NULL" for k in ("depth", "normal", "residual", "status", "rgba")},
                          zero_ok={"n_hits": None}),
    "disn_mesh_components": E("nf=1 nv=3", "connectivity=0", host={"faces_host": TRI_F, "labels_host": ("i", [0])},
                              zero_ok={"nf": 0, "nv": None},
                              no_extreme={"nf": "faces_host holds nf rows"}),
    "disn_voxel_grid_words": Q("n=4"),
    "disn_voxel_surface_workspace_bytes": Q("nf=1", zero_ok=("nf",)),
    "disn_voxel_surface": E("nv=3 nf=1 dim=4 nkeys=4", "kmin=-2", _ws("disn_voxel_surface_workspace_bytes(nf)"),
                            zero_ok={"nf": None, "nv": None}),
    "disn_voxel_fill_workspace_bytes": Q("n=4"),
    "disn_voxel_fill": E("n=4", need=_ws("disn_voxel_fill_workspace_bytes(n)")),
    "disn_voxel_index_grid": E("nkeys=4 dim=4"),
    "disn_voxel_iou": E("nviews=1 words=2"),
    "disn_assemble_batch": E("n_obj=1 n_view=1 B=1 S=4", "rot=0 backcolorwhite=0",
                             nullable={"rot_all": "may be NULL when rot = 0"}),
    "disn_metrics_workspace_bytes": Q("b=1 n=1 m=1"),
    "disn_nn_distance": E("b=1 n=1 m=1", need=_ws("disn_metrics_workspace_bytes(b,n,m)")),
    "disn_approx_match": E("b=1 n=1 m=1", need=_ws("disn_metrics_workspace_bytes(b,n,m)")),
    "disn_match_cost": E("b=1 n=1 m=1", need=_ws("disn_metrics_workspace_bytes(b,n,m)")),
    "disn_emd": E("b=1 n=1 m=1", need=_ws("disn_metrics_workspace_bytes(b,n,m)")),
    "disn_grid_points": E(**GRID),
    "disn_query_grid_workspace_bytes": Q("max_points=125"),
    "disn_query_grid": E(need=_ws("disn_query_grid_workspace_bytes(k1)"), **GRID),
    "disn_fold_local": E(need=_ws("disn_fold_local_workspace_bytes()")),
    "disn_query_folded": E("B=1 N=8", need=_ws("disn_query_workspace_bytes(B,N)")),
    "disn_query_grid_folded": E(need=_ws("disn_query_grid_workspace_bytes(k1)"), **GRID),
    "disn_gather_taps_pool": E("V=1 N=4", "pool=0", nullable={"weights": "NULL: every w_v = 1 / V"}),
    "disn_pool_embedding": E("V=1", "pool=0", nullable={"weights": "NULL: every w_v = 1 / V"}),
    "disn_query_views_workspace_bytes": Q("N=8"),
    "disn_query_views": E("V=1 N=8", "pool=0", _ws("disn_query_views_workspace_bytes(N)"),
                          nullable={"weights": "NULL: every w_v = 1 / V"}),
    "disn_query_grid_views_workspace_bytes": Q("R=4"),
    "disn_query_grid_views": E("V=1 R=4 k1=125", "pool=0 k0=0", _ws("disn_query_grid_views_workspace_bytes(R)"),
                               nullable={"weights": "NULL: every w_v = 1 / V"}),
    "disn_query_grad_workspace_bytes": Q("B=1 N=4"),
    "disn_query_grad": E("B=1 N=4", need=_ws("disn_query_grad_workspace_bytes(B,N)"),
                         nullable={"sdf": "sdf [B,N] (un-divided pred_sdf; may be NULL)"}),
    "disn_mesh_clean_workspace_bytes": Q("B=1 nv_total=3 nf_total=1", zero_ok=MESH_Q),
    "disn_mesh_components_device": E("B=1", "connectivity=0", _ws("disn_mesh_clean_workspace_bytes(B,3,1)"), MESH_HOST,
                                     nullable={"comp_verts": "comp_verts (optional, int64 [sum nf] capacity, needs verts)",
                                               "verts": "comp_verts (optional, ..., needs verts): only then"},
                                     no_extreme=MESH_B),
    "disn_mesh_clean_count_batch": E("B=1", "connectivity=0 dist_thresh=0.5 num_thresh=0.5",
                                     _ws("disn_mesh_clean_workspace_bytes(B,3,1)"), MESH_HOST, no_extreme=MESH_B),
    "disn_mesh_clean_emit_batch": E("B=1", need=_ws("disn_mesh_clean_workspace_bytes(B,3,1)"),
                                    host=dict(MESH_HOST, counts_host=("q", [1, 1, 3, 1, 0])), no_extreme=MESH_B),
    # ---- include/disn_amd_simplify.h
    "disn_mesh_simplify_workspace_bytes": Q("B=1 nv_total=3 nf_total=1", zero_ok=MESH_Q),
    "disn_mesh_simplify_count_batch": E("B=1", "dedup=1", _ws("disn_mesh_simplify_workspace_bytes(B,3,1)"),
                                        dict(MESH_HOST, lattice_host=("d", [-1, -1, -1, 0.5]), cells_host=("i", [4])),
                                        no_extreme=MESH_B),
    "disn_mesh_simplify_emit_batch": E("B=1", need=_ws("disn_mesh_simplify_workspace_bytes(B,3,1)"),
                                       host=dict(MESH_HOST, sizes_host=("q", [3, 1, 0, 0, 0, 0, 0, 0])), no_extreme=MESH_B),
    # ---- include/disn_amd_colour.h
    "disn_mesh_colour_workspace_bytes": Q("B=1 V=1 nv_total=3 nf_total=1 S=1", zero_ok=MESH_Q),
    "disn_mesh_zbuffer_batch": E("B=1 V=1 S=1", need=_ws("disn_mesh_colour_workspace_bytes(B,V,3,1,S)"), host=MESH_HOST,
                                 no_extreme=MESH_B),
    "disn_mesh_colour_batch": E("B=1 V=1 S=1", "rel_tol=0.01 mirror_axis=-1 fill_iters=0 bgr=0",
                                _ws("disn_mesh_colour_workspace_bytes(B,V,3,1,S)"), MESH_HOST,
                                nullable={"alpha": "uint8 or NULL (device)"}, no_extreme=MESH_B),
    "disn_write_obj_colours": E("nv=3 nf=1", host={"verts": TRI_V, "colours": ("B", [0] * 9), "normals": TRI_V,
                                                   "faces": TRI_F}, zero_ok={"nv": 0, "nf": 0},
                                nullable={"normals": "with normals \"vn\" lines"},
                                no_extreme={"nv": "verts holds nv rows", "nf": "faces holds nf rows"}),
    # ---- include/disn_amd_sample.h
    "disn_mesh_sample_workspace_bytes": Q("B=1 nv_total=3 nf_total=1 n=4", zero_ok=MESH_Q),
    "disn_mesh_sample_batch": E("B=1 n=4", need=_ws("disn_mesh_sample_workspace_bytes(B,3,1,n)"),
                                host=dict(MESH_HOST, seeds_host=("Q", [1])),
                                nullable={"normals": "normals [B][n][3] float32 or NULL",
                                          "face_idx": "face_idx [B][n] int32 (local to the mesh) or NULL"},
                                no_extreme=MESH_B),
    # ---- include/disn_amd_smooth.h
    "disn_mesh_smooth_workspace_bytes": Q("B=1 nv_total=3 nf_total=1", zero_ok=MESH_Q),
    "disn_mesh_smooth_batch": E("B=1 iters=1", "lam=0.5 mu=-0.5 pin_boundary=0",
                                _ws("disn_mesh_smooth_workspace_bytes(B,3,1)"),
                                dict(MESH_HOST, max_move_host=("d", [-1.0])),
                                nullable={"max_move_host": "max_move_host == NULL: no cap"}, no_extreme=MESH_B),
}


def check_complete(protos=None):
    protos = protos or parse_headers()
    listed = set(CASES) | set(NO_MUTATION)
    assert not set(CASES) & set(NO_MUTATION)
    assert not listed - set(protos), "not declared in any header: %s" % sorted(listed - set(protos))
    assert not set(protos) - listed, "declared without a CASE: %s" % sorted(set(protos) - listed)
    for name in NO_MUTATION:
        assert not protos[name].params or name == "disn_crc32c", name


# ---------------------------------------------------------------- the calls --------------------------------------
OBJ_BY_BINDING = {"VggWeights": "vgg", "MlpWeights": "mlp", "CamWeights": "cam", "EqWeights": "eq", "ParamLayout": "layout",
                  "CamParamLayout": "cam_layout", "c_void_p_Array_5": "taps5", "c_double_Array_6": "box6",
                  "c_float_Array_9": "k9", "c_void_p": "slot", "c_long": "slot"}


def is_query(proto):
    return proto.ret == "size_t"


def _maximum(cls):
    return INT_MAX if cls == "int" else INT64_MAX


def _need_token(case, expr, delta):
    m = re.match(r"^(disn_\w+)\((.*)\)$", expr)
    args = [int(eval(a, {}, dict(case.sizes))) for a in m.group(2).split(",")] if m.group(2).strip() else []
    return ("need", m.group(1), args, delta)


def base_args(proto, case, argtypes):
    """the CASE as a list of tokens (never called as it stands)"""
    import ctypes as C
    out = []
    for (ctype, pname), at in zip(proto.params, argtypes):
        cls = c_class(ctype)
        if cls in ("int", "int64_t"):
            assert (pname in case.sizes) != (pname in case.flags), "%s: %s is neither a size nor a flag" % (proto.name, pname)
            out.append(case.sizes.get(pname, case.flags.get(pname)))
        elif cls in ("float", "double"):
            out.append(float(case.flags.get(pname, 1.0)))
        elif cls == "size_t":
            assert pname in case.need, "%s: no query sizes %s" % (proto.name, pname)
            out.append(_need_token(case, case.need[pname][1], 0))
        elif cls == "uint32_t":
            out.append(int(case.flags.get(pname, 0)))
        elif pname in case.nullable:
            out.append(("null",))                      # the smallest legal call leaves out what it may
        elif pname in case.host:
            out.append(("host",) + tuple(case.host[pname]))
        elif at is C.c_char_p:
            out.append(("obj", "path"))
        elif isinstance(at, type(C.POINTER(C.c_int))):
            out.append(("obj", OBJ_BY_BINDING[at._type_.__name__]))
        elif pname == "stream" and pname not in case.required:
            out.append(("null",))
        else:
            assert not pname.endswith("_host"), "%s: host pointer %s needs real memory" % (proto.name, pname)
            out.append(("fake",))
    return out


def calls_for(name, protos, sig):
    """every mutated call of one entry"""
    proto, case = protos[name], CASES[name]
    base = base_args(proto, case, sig[name][1])
    idx = {pname: i for i, (_, pname) in enumerate(proto.params)}
    cls = {pname: c_class(ctype) for ctype, pname in proto.params}
    assert set(case.sizes) | set(case.flags) | set(case.need) | set(case.host) | set(case.nullable) <= set(idx), \
        "%s: the CASE names a parameter the prototype does not have" % name
    for p in case.sizes:
        assert cls[p] in ("int", "int64_t"), (name, p)

    def mutated(**kw):
        a = list(base)
        for k, v in kw.items():
            a[idx[k]] = v
        return a

    extreme = {p: _maximum(cls[p]) for p in case.sizes if p not in case.no_extreme}
    # The type's maximum is odd: a parameter with a divisibility rule (Cin % 32, N % 256 ...) is refused for that alone,
    # before any bound or product is formed.  So every size also takes the largest multiple of 256 of its type: alone,
    # with the sizes that have no such rule at 1 (so that no other operand refuses the call first), and all such sizes at
    # once.  A size "has a rule" where the CASE's own value is a multiple of 32.
    ruled = [p for p in extreme if case.sizes[p] % 32 == 0]
    ones = {p: 1 for p in extreme if p not in ruled}
    aligned = []
    for p, v in extreme.items():
        aligned.append(("%s=aligned max" % p, {p: v & ~255}))
        if ones and set(ones) != {p}:
            aligned.append(("%s=aligned max, unruled sizes=1" % p, dict({q: 1 for q in ones if q != p}, **{p: v & ~255})))
    if len(ruled) > 1:
        aligned.append(("every ruled size=aligned max, the others=1", dict(ones, **{p: extreme[p] & ~255 for p in ruled})))
    if is_query(proto):
        case_value = ("need", name, list(base), 0)
        for p in case.sizes:
            if p not in case.zero_ok:
                yield Call(name, "%s=0" % p, mutated(**{p: 0}), ("zero",))
            yield Call(name, "%s=-1" % p, mutated(**{p: -1}), ("zero",))
        if case.positive:
            yield Call(name, "the CASE", list(base), ("pos",))
        for p, v in extreme.items():
            yield Call(name, "%s=max" % p, mutated(**{p: v}), ("zero_or_ge", case_value))
        if len(extreme) > 1:
            yield Call(name, "every size=max", mutated(**extreme), ("zero_or_ge", case_value))
        for label, kw in aligned:
            yield Call(name, label, mutated(**kw), ("zero_or_ge", case_value))
        return
    sized = {ptr: nbytes for nbytes, (ptr, _) in case.need.items()}
    for ctype, p in proto.params:
        if cls[p] != "pointer" or p in case.nullable or (p == "stream" and p not in case.required):
            continue
        if p in sized:
            yield Call(name, "%s=NULL" % p, mutated(**{p: ("null",)}), ("neg_if_need", base[idx[sized[p]]]))
        else:
            yield Call(name, "%s=NULL" % p, mutated(**{p: ("null",)}), ("eq", E_ARG))
    for p in case.sizes:
        if p not in case.zero_ok:
            yield Call(name, "%s=0" % p, mutated(**{p: 0}), ("neg",))
        elif case.zero_ok[p] is not None:
            yield Call(name, "%s=0" % p, mutated(**{p: 0}), ("eq", case.zero_ok[p]))
        yield Call(name, "%s=-1" % p, mutated(**{p: -1}), ("neg",))
    for nbytes, (ptr, expr) in case.need.items():
        yield Call(name, "%s=need-1" % nbytes, mutated(**{nbytes: _need_token(case, expr, -1)}), ("eq_if_need", E_WS))
    big = {nbytes: ("big",) for nbytes in case.need}
    for p, v in extreme.items():
        yield Call(name, "%s=max" % p, mutated(**dict(big, **{p: v})), ("neg",))
    if len(extreme) > 1:
        yield Call(name, "every size=max", mutated(**dict(big, **extreme)), ("neg",))
    for label, kw in aligned:
        yield Call(name, label, mutated(**dict(big, **kw)), ("neg",))


def all_calls(protos=None):
    protos = protos or parse_headers()
    sig = binding()
    for name in sorted(CASES):
        for c in calls_for(name, protos, sig):
            yield c
