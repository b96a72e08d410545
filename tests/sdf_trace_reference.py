"""Float32 numpy restatement of disn_amd/csrc/sdf_trace.hip (setup / advance / collect / shade), operation for operation,
and a float64 closed form for ray - sphere.  The kernels are compiled with -ffp-contract=off and compared with this bit
for bit (tests/test_gpu_sdf_trace.py); tests/test_sdf_trace_host.py runs it alone on analytic fields.

The state is a dict of [n] arrays named as disn_amd.ops.TRACE_FIELDS; lists of rays are ascending int64 arrays (the
device's order is unspecified: compare as sets, or per ray)."""
import numpy as np

f32 = np.float32
MARCH, BRACKET, DONE = 0, 1, 2
DEFAULTS = dict(iso=0.0, sdf_weight=1.0, eps=1e-4, step_scale=0.8, min_step=1e-3, max_step=0.1, max_steps=96, refine=8)
FLOAT_FIELDS = ("t", "t1", "len", "t_lo", "f_lo", "t_hi", "f_hi")
INT_FIELDS = ("phase", "status", "march_evals", "bracket_evals", "have_lo", "hit_slot")


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def rays(cams, H, W):
    """-> (org [n,3], dir [n,3]) float32 of cams [V,12], ray r = (v*H + i)*W + j at x = j + 0.5, y = i + 0.5"""
    cams = np.asarray(cams, f32).reshape(-1, 12)
    V = cams.shape[0]
    x = (np.arange(W).astype(f32) + f32(0.5))[None, None, :, None]
    y = (np.arange(H).astype(f32) + f32(0.5))[None, :, None, None]
    d0, dx, dy = (cams[:, None, None, k:k + 3] for k in (3, 6, 9))
    d = (d0 + x * dx) + y * dy
    org = np.broadcast_to(cams[:, None, None, 0:3], d.shape)
    return np.ascontiguousarray(org.reshape(V * H * W, 3)), np.ascontiguousarray(d.reshape(V * H * W, 3))


def points(org, d, t, which):
    """org + t * dir of the rays ``which`` -> [len(which),3] float32"""
    return (org[which] + t[which, None] * d[which]).astype(f32)


def setup(cams, H, W, box, t_min=0.0):
    """-> (state, active rays); box = 6 host doubles, cast to float32"""
    org, d = rays(cams, H, W)
    n = org.shape[0]
    box = np.asarray([float(v) for v in box], np.float64).astype(f32)
    tn = np.full(n, f32(t_min), f32)
    tf = np.full(n, np.inf, f32)
    miss = np.zeros(n, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            lo, hi = box[a] - org[:, a], box[a + 3] - org[:, a]
            par = np.abs(d[:, a]) < f32(2.0 ** -100)
            miss |= par & ((lo > 0) | (hi < 0))
            inv = f32(1.0) / np.where(par, f32(1.0), d[:, a])
            ta, tb = lo * inv, hi * inv
            tn = np.where(par, tn, np.fmax(tn, np.fmin(ta, tb)))
            tf = np.where(par, tf, np.fmin(tf, np.fmax(ta, tb)))
    ln = np.sqrt(dot(d, d)).astype(f32)
    keep = ~miss & (tn <= tf) & (tf < np.inf) & (ln > 0)
    z = np.zeros(n, f32)
    st = {"t": np.where(keep, tn, z), "t1": np.where(keep, tf, z), "len": ln, "t_lo": z.copy(), "f_lo": z.copy(),
          "t_hi": z.copy(), "f_hi": z.copy(), "phase": np.where(keep, MARCH, DONE).astype(np.int32)}
    for k in ("status", "march_evals", "bracket_evals", "have_lo"):
        st[k] = np.zeros(n, np.int32)
    st["hit_slot"] = np.full(n, -1, np.int32)
    st["org"], st["dir"] = org, d
    return st, np.nonzero(keep)[0]


def false_position(t_lo, f_lo, t_hi, f_hi):
    w = t_hi - t_lo
    den = f_lo - f_hi
    q = (w * f_lo) / den
    m = f32(0.05) * w
    return np.fmin(np.fmax(t_lo + q, t_lo + m), t_hi - m)


def advance(st, active, values, **params):
    """one iteration: ``values`` [len(active)] float32 of the active rays' points -> the next active rays"""
    p = dict(DEFAULTS, **params)
    eps, scale, smin, smax = (f32(p[k]) for k in ("eps", "step_scale", "min_step", "max_step"))
    nxt = []
    for r, v in zip(np.asarray(active).tolist(), np.asarray(values, f32)):
        f = v / f32(p["sdf_weight"]) - f32(p["iso"])
        t = st["t"][r]
        phase = st["phase"][r]
        status, done = 0, False
        if np.abs(f) <= eps:
            status, done = 1, True
        elif phase == MARCH:
            st["march_evals"][r] += 1
            if f < 0:
                if not st["have_lo"][r]:
                    status, done = 2, True
                else:
                    st["t_hi"][r], st["f_hi"][r], st["phase"][r] = t, f, BRACKET
                    t = false_position(st["t_lo"][r], st["f_lo"][r], t, f)
            else:
                st["t_lo"][r], st["f_lo"][r], st["have_lo"][r] = t, f, 1
                if t >= st["t1"][r]:
                    status, done = 0, True
                elif st["march_evals"][r] >= p["max_steps"]:
                    status, done = 4, True
                else:
                    step = np.fmin(np.fmax(scale * f, smin), smax)
                    t = np.fmin(t + step / st["len"][r], st["t1"][r])
        elif phase == BRACKET:
            st["bracket_evals"][r] += 1
            if f < 0:
                st["t_hi"][r], st["f_hi"][r] = t, f
            else:
                st["t_lo"][r], st["f_lo"][r] = t, f
            if st["bracket_evals"][r] >= p["refine"]:
                status, done = 3, True
            else:
                t = false_position(st["t_lo"][r], st["f_lo"][r], st["t_hi"][r], st["f_hi"][r])
        else:
            status, done = int(st["status"][r]), True
        if done:
            st["phase"][r], st["status"][r] = DONE, status
        else:
            assert isinstance(t, f32), type(t)
            st["t"][r] = t
            nxt.append(r)
    return np.asarray(nxt, np.int64)


def collect(st):
    """-> the hit rays (status 1..3), ascending; sets hit_slot to a ray's position in that list (the device's slots
    are its own list's: compare through the list)"""
    hit = (st["phase"] == DONE) & (st["status"] >= 1) & (st["status"] <= 3)
    which = np.nonzero(hit)[0]
    st["hit_slot"][:] = -1
    st["hit_slot"][which] = np.arange(which.size, dtype=np.int32)
    return which


def shade(st, hits, pred, grad, iso=0.0, sdf_weight=1.0, ambient=0.3):
    """pred [len(hits)], grad [len(hits),3] float32 -> {"depth", "normal", "residual", "status", "rgba"} as [n] / [n,k]"""
    n = st["t"].shape[0]
    out = {"depth": np.zeros(n, f32), "normal": np.zeros((n, 3), f32), "residual": np.zeros(n, f32),
           "status": st["status"].astype(np.uint8), "rgba": np.zeros((n, 4), np.uint8)}
    if len(hits) == 0:
        return out
    pred, g = np.asarray(pred, f32), np.asarray(grad, f32).reshape(-1, 3)
    d = st["dir"][hits]
    amb = f32(ambient)
    out["depth"][hits] = st["t"][hits]
    out["residual"][hits] = np.abs(pred / f32(sdf_weight) - f32(iso))
    g2 = dot(g, g)
    gl = np.sqrt(g2).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = (g / gl[:, None]).astype(f32)
        den = gl * np.sqrt(dot(d, d)).astype(f32)
        c = np.where(den > 0, np.fmin(np.abs(dot(g, d)) / den, f32(1.0)), f32(0.0)).astype(f32)
    out["normal"][hits] = np.where((g2 < f32(1e-12))[:, None], f32(0.0), nrm)
    sh = amb + (f32(1.0) - amb) * c
    b = np.fmin(np.floor(sh * f32(0.8) * f32(255.0) + f32(0.5)), f32(255.0)).astype(np.uint8)
    out["rgba"][hits] = np.stack([b, b, b, np.full_like(b, 255)], axis=1)
    return out


def trace(field, cams, H, W, box, grad=None, t_min=0.0, ambient=0.3, **params):
    """the whole loop on the host -> (state, outputs of shade, stats)"""
    st, active = setup(cams, H, W, box, t_min)
    stats = {"rays": st["t"].shape[0], "box_rays": int(active.size), "evaluations": 0, "iterations": 0, "hits": 0}
    while active.size:
        vals = field(points(st["org"], st["dir"], st["t"], active))
        stats["evaluations"] += int(active.size)
        stats["iterations"] += 1
        active = advance(st, active, vals, **params)
    hits = collect(st)
    stats["hits"] = int(hits.size)
    hp = points(st["org"], st["dir"], st["t"], hits)
    p = dict(DEFAULTS, **params)
    g = grad(hp) if grad is not None else np.zeros_like(hp)
    out = shade(st, hits, field(hp) if hits.size else np.zeros(0, f32), g, p["iso"], p["sdf_weight"], ambient)
    return st, out, stats


# ---- analytic fields (float32, negative inside) ------------------------------------------------------------------
CENTRE = np.asarray([0.1, -0.05, 0.02], f32)
RADIUS = f32(0.4)


def sphere(p, scale=1.0, offset=0.0):
    q = np.asarray(p, f32) - CENTRE
    return ((np.sqrt(dot(q, q)).astype(f32) - RADIUS) * f32(scale) + f32(offset)).astype(f32)


def sphere_grad(p, scale=1.0):
    q = np.asarray(p, f32) - CENTRE
    return (q / np.sqrt(dot(q, q)).astype(f32)[:, None] * f32(scale)).astype(f32)


def torus(p, R=0.45, r=0.15):
    """about the y axis through CENTRE"""
    q = np.asarray(p, f32) - CENTRE
    a = np.sqrt(q[:, 0] * q[:, 0] + q[:, 2] * q[:, 2]).astype(f32) - f32(R)
    return (np.sqrt(a * a + q[:, 1] * q[:, 1]).astype(f32) - f32(r)).astype(f32)


def torus_grad(p, R=0.45, r=0.15):
    q = np.asarray(p, f32) - CENTRE
    rho = np.sqrt(q[:, 0] * q[:, 0] + q[:, 2] * q[:, 2]).astype(f32)
    a = rho - f32(R)
    ln = np.sqrt(a * a + q[:, 1] * q[:, 1]).astype(f32)
    return np.stack([a * q[:, 0] / rho / ln, q[:, 1] / ln, a * q[:, 2] / rho / ln], axis=1).astype(f32)


def constant(value):
    return lambda p: np.full(np.asarray(p).shape[0], value, f32)


# ---- float64 closed form -----------------------------------------------------------------------------------------
def ray_sphere(org, d, radius, centre=CENTRE):
    """float64: (b [n] impact parameter, s [n] distance ALONG THE UNIT ray of the near intersection with the sphere of
    ``radius``, NaN where the line misses it, ou [n] = o.u).  A distance s is t = s / |dir| in the ray's parameter."""
    o = np.asarray(org, np.float64) - np.asarray(centre, np.float64)
    d = np.asarray(d, np.float64)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    ou = (o * u).sum(axis=1)
    b2 = (o * o).sum(axis=1) - ou * ou
    b = np.sqrt(np.maximum(b2, 0.0))
    with np.errstate(invalid="ignore"):
        s = -ou - np.sqrt(float(radius) ** 2 - b2)
    return b, s, ou
