"""The host half of every C entry, swept from one table (tests/abi_table.py): a NULL required pointer is DISN_E_ARG, a
non-positive size is refused, a workspace one byte short is DISN_E_WS, a size at the top of its type is refused (entries)
or answered with 0 (size queries).  Every call here is one the entry must refuse BEFORE anything is enqueued; the sweep
runs in one fresh child process with the device hidden, so a call that slips through a missing check meets
hipErrorNoDevice (a positive status: a failure that names the entry) and can never reach a GPU with fake pointers.

    python tests/test_abi_errors_host.py --child [--only ENTRY]    # what the child runs: `CALL entry / mutation` before each
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [p for p in (HERE, ROOT) if p not in sys.path]

import abi_table as T  # noqa: E402

CODES = {"f": C.c_float, "d": C.c_double, "i": C.c_int32, "q": C.c_int64, "Q": C.c_uint64, "B": C.c_uint8}


# ---------------------------------------------------------------- the child --------------------------------------
def device_count():
    """hipGetDeviceCount through the runtime the library itself is linked against"""
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            hip = None
    assert hip is not None, "cannot load the HIP runtime to count the devices"
    n = C.c_int(-1)
    rc = hip.hipGetDeviceCount(C.byref(n))
    return 0 if rc != 0 else n.value


class Materialiser:
    def __init__(self, lib, tmp):
        self.lib, self.tmp, self.keep = lib, tmp, []

    def obj(self, kind, argtype):
        from disn_amd import _lib
        if kind == "path":
            return os.path.join(self.tmp, "sweep.obj").encode()
        o = argtype._type_()
        if kind in ("vgg", "mlp", "cam", "eq"):
            for fname, ftype in o._fields_:
                if ftype is C.c_void_p:
                    setattr(o, fname, T.FAKE)
                elif ftype is C.c_int:
                    setattr(o, fname, 1024 if fname == "num_classes" else 0)
                else:                                       # arrays of pointers, possibly nested
                    flat = (C.c_void_p * (C.sizeof(ftype) // C.sizeof(C.c_void_p))).from_buffer(getattr(o, fname))
                    for i in range(len(flat)):
                        flat[i] = T.FAKE
        elif kind == "taps5":
            o[:] = [T.FAKE] * 5
        elif kind == "box6":
            o[:] = [-1, -1, -1, 1, 1, 1]
        elif kind == "k9":
            o[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        else:
            assert kind in ("layout", "cam_layout", "slot"), kind
        self.keep.append(o)
        assert isinstance(o, (_lib.VggWeights, _lib.MlpWeights, _lib.CamWeights, _lib.EqWeights, _lib.ParamLayout,
                              _lib.CamParamLayout, C.Array, C.c_void_p, C.c_int64))
        return C.byref(o)

    def value(self, tok, argtype):
        if not isinstance(tok, (tuple, list)):
            return tok
        kind = tok[0]
        if kind == "null":
            return None
        if kind == "fake":
            return T.FAKE
        if kind == "host":
            buf = (CODES[tok[1]] * len(tok[2]))(*tok[2])
            self.keep.append(buf)
            return C.cast(buf, C.c_void_p)
        if kind == "obj":
            return self.obj(tok[1], argtype)
        if kind == "need":
            return getattr(self.lib, tok[1])(*[self.value(a, None) for a in tok[2]]) + tok[3]
        assert kind == "big", tok
        return 1 << 62


def judge(r, expect, mat):
    """None when the call need not be made / the result is right, else what was expected"""
    kind = expect[0]
    if kind == "eq":
        return None if r == expect[1] else "expected %d" % expect[1]
    if kind in ("neg", "neg_if_need"):
        return None if r < 0 else "expected a negative status"
    if kind == "eq_if_need":
        return None if r == expect[1] else "expected %d" % expect[1]
    if kind == "zero":
        return None if r == 0 else "expected 0"
    if kind == "pos":
        return None if r > 0 else "expected > 0"
    assert kind == "zero_or_ge", kind
    least = mat.value(expect[1], None)
    return None if r == 0 or r >= least else "expected 0 or at least the CASE's %d" % least


def child():
    from disn_amd import _lib
    lib = _lib.lib()
    n = device_count()
    if n != 0:
        print("REFUSED: %d device(s) visible -- the sweep only runs with the device hidden" % n, flush=True)
        return 3
    sig = T.binding()
    failures, skipped, ncalls = [], [], 0
    with tempfile.TemporaryDirectory() as tmp:
        only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
        for call in T.all_calls():
            if only and call.entry != only:
                continue
            mat = Materialiser(lib, tmp)
            kind = call.expect[0]
            if kind in ("neg_if_need", "eq_if_need"):
                i = [k for k, a in enumerate(call.args) if isinstance(a, tuple) and a[0] == "need"][0]
                if mat.value(call.args[i][:3] + (0,), None) == 0:
                    skipped.append([call.entry, call.label, "the CASE needs no workspace"])
                    continue
            args = [mat.value(a, at) for a, at in zip(call.args, sig[call.entry][1])]
            print("CALL %s / %s" % (call.entry, call.label), flush=True)
            r = getattr(lib, call.entry)(*args)
            ncalls += 1
            why = judge(r, call.expect, mat)
            if why is None:
                continue
            if r > 0 and sig[call.entry][0] is C.c_int:
                why += " -- a positive status: no check stopped the call before the runtime did"
            failures.append([call.entry, call.label, int(r), why])
    print("RESULT " + json.dumps({"calls": ncalls, "failures": failures, "skipped": skipped}), flush=True)
    return 0


# ---------------------------------------------------------------- the parent -------------------------------------
@functools.lru_cache(maxsize=None)
def sweep():
    from disn_amd.csrc import build
    build.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    lines = r.stdout.splitlines()
    result = [l for l in lines if l.startswith("RESULT ")]
    if r.returncode != 0 or not result:
        last = [l for l in lines if l.startswith("CALL ")]
        pytest.fail("the sweep's child ended with status %d %s\n%s\n%s" % (
            r.returncode, "in " + last[-1][5:] if last else "before its first call", "\n".join(lines[-3:]),
            r.stderr[-2000:]))
    return json.loads(result[0][7:])


def test_the_table_matches_the_headers_and_the_binding():
    protos = T.parse_headers()
    assert len(T.header_paths()) == 5 and len(protos) == sum(len(t) for t in T.binding_tables())
    T.check_against_binding(protos)
    T.check_complete(protos)
    calls = list(T.all_calls(protos))
    assert {c.entry for c in calls} == set(T.CASES)        # every CASE has something to mutate
    labels = [(c.entry, c.label) for c in calls]
    assert len(labels) == len(set(labels))


def test_the_sweep_made_every_call():
    res = sweep()
    planned = list(T.all_calls())
    assert res["calls"] + len(res["skipped"]) == len(planned) and res["calls"] > 10 * len(T.CASES)
    # every CASE that takes a workspace is at a shape that needs one, so no short-workspace call is left out
    assert not res["skipped"], res["skipped"]


@pytest.mark.parametrize("entry", sorted(T.CASES))
def test_entry_refuses_every_mutated_call(entry):
    bad = [f for f in sweep()["failures"] if f[0] == entry]
    assert not bad, "\n".join("%s / %s returned %d: %s" % tuple(f) for f in bad)


if __name__ == "__main__":
    sys.exit(child() if "--child" in sys.argv else 2)
