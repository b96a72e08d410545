"""The guard-band helper (tests/guarded_alloc.py) on CPU tensors, and the header coverage of the memory-contract table
(tests/test_gpu_memory_contract.py): every entry of every header under include/ is either run under guards -- by a
scenario, or for the mesh modules' own headers by the test their file names -- or exempt because it writes no device
memory and launches nothing."""
import ast
import glob
import os
import re

import numpy as np
import pytest
import torch

import guarded_alloc as GA
from guarded_alloc import GuardError, guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(g, t):
    (r,) = [r for r in g.records if r.buf.data_ptr() + r.start == t.data_ptr()]
    return r


# the call forms of torch.empty under disn_amd/ (grep "torch.empty("): a tuple, varargs (voxel.py `torch.empty(2, V,`),
# a bare int (`torch.empty(need,`, `torch.empty(max(int(nbytes), 256),`), a numpy shape tuple (data_resident.py
# `torch.empty(a.shape,`), a dtype looked up by name (`getattr(torch, str(a.dtype))`) -- always with dtype= and device=
@pytest.mark.parametrize("variant", ["A", "B"])
def test_every_call_form_of_empty(variant):
    a = np.zeros((3, 5, 2), np.int16)
    forms = [
        (lambda: torch.empty((4, 7), dtype=torch.float32, device="cpu"), (4, 7), torch.float32),
        (lambda: torch.empty((9,), dtype=torch.float32, device=torch.device("cpu")), (9,), torch.float32),
        (lambda: torch.empty(2, 3, dtype=torch.int64, device="cpu"), (2, 3), torch.int64),
        (lambda: torch.empty(11, dtype=torch.uint8, device="cpu"), (11,), torch.uint8),
        (lambda: torch.empty(max(int(7), 256), dtype=torch.uint8, device="cpu"), (256,), torch.uint8),
        (lambda: torch.empty(a.shape, dtype=getattr(torch, str(a.dtype)), device="cpu"), (3, 5, 2), torch.int16),
        (lambda: torch.empty([2, 2], dtype=torch.int32, device="cpu"), (2, 2), torch.int32),
        (lambda: torch.empty(torch.Size((5, 1)), dtype=torch.float64, device="cpu"), (5, 1), torch.float64),
        (lambda: torch.empty(np.int64(6), dtype=torch.float32, device="cpu"), (6,), torch.float32),
        (lambda: torch.empty(size=(3, 3), dtype=torch.float32, device="cpu"), (3, 3), torch.float32),
        (lambda: torch.empty(5), (5,), torch.get_default_dtype()),
    ]
    guard, poison = GA.VARIANTS[variant]
    with guarded(variant, cpu=True) as g:
        for make, shape, dtype in forms:
            t = make()
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
            assert t.data_ptr() % 256 == 0
            r = _record(g, t)
            assert r.nbytes == t.numel() * t.element_size()
            assert r.start >= GA.GUARD_BYTES and r.buf.numel() - r.start - r.nbytes >= GA.GUARD_BYTES
            assert GA.GUARD_BYTES % 256 == 0 and GA.GUARD_BYTES >= 4096
            assert (r.buf[r.start:r.start + r.nbytes] == poison).all()          # poison in the payload
            assert (r.buf[:r.start] == guard).all() and (r.buf[r.start + r.nbytes:] == guard).all()
        g.check()
        assert len(g.records) == len(forms)


def test_poison_values_and_the_two_variants_differ():
    seen = {}
    for variant in ("A", "B"):
        with guarded(variant, cpu=True):
            f = torch.empty(4, dtype=torch.float32, device="cpu")
            i = torch.empty(4, dtype=torch.int32, device="cpu")
            seen[variant] = (f.clone(), i.clone())
    assert torch.isnan(seen["A"][0]).all() and (seen["A"][1] == -1).all()
    assert (seen["B"][0] > 3.3e38).all() and torch.isfinite(seen["B"][0]).all() and (seen["B"][1] == 0x7F7F7F7F).all()
    (ga, pa), (gb, pb) = GA.VARIANTS["A"], GA.VARIANTS["B"]
    assert ga != gb and pa != pb and 0 not in (ga, pa, gb, pb)


def test_zeros_full_and_empty_like_keep_their_contents():
    with guarded("A", cpu=True) as g:
        z = torch.zeros((3, 4), dtype=torch.int64, device="cpu")
        z1 = torch.zeros(5, dtype=torch.float32, device="cpu")
        f = torch.full((2, 3), 7.5, dtype=torch.float32, device="cpu")
        fi = torch.full((4,), 3, device="cpu")
        fk = torch.full((4,), fill_value=-2, dtype=torch.int32, device="cpu")
        e = torch.empty_like(z1)
        ed = torch.empty_like(z, dtype=torch.uint8)
        assert z.shape == (3, 4) and z.dtype == torch.int64 and not z.any() and not z1.any()
        assert (f == 7.5).all() and f.shape == (2, 3)
        assert fi.dtype == torch.int64 and (fi == 3).all() and fk.dtype == torch.int32 and (fk == -2).all()
        assert e.shape == z1.shape and e.dtype == torch.float32 and torch.isnan(e).all()
        assert ed.shape == z.shape and ed.dtype == torch.uint8 and (ed == 0xFF).all()
        assert len(g.records) == 7                   # all seven sit between guards
        g.check()


def test_what_is_not_substituted():
    with guarded("A") as g:                          # the default: CUDA allocations only
        t = torch.empty((4,), dtype=torch.float32, device="cpu")
        assert not g.records and t.shape == (4,)
    with guarded("A", cpu=True) as g:
        assert torch.empty(0, dtype=torch.float32, device="cpu").numel() == 0        # nothing to guard
        assert torch.empty((2, 0), dtype=torch.float32, device="cpu").shape == (2, 0)
        out = torch.zeros(3)
        assert torch.empty(3, out=out) is out          # an out= call passes through
        assert len(g.records) == 1                   # only `out = torch.zeros(3)`


@pytest.mark.parametrize("variant", ["A", "B"])
def test_a_byte_before_and_a_byte_after_the_payload_are_reported(variant):
    with guarded(variant, cpu=True) as g:
        t = torch.empty((5, 3), dtype=torch.float32, device="cpu")        # 60 bytes: 4 bytes of padding to 16
        r = _record(g, t)
        g.check()
        r.buf[r.start - 1] = 0                       # plain indexing into the underlying buffer: inside the allocation
        with pytest.raises(GuardError) as e:
            g.check()
        msg = str(e.value)
        assert "before the payload" in msg and "offset -1 " in msg and "1 byte(s)" in msg
        assert "(5, 3) float32" in msg and "test_guarded_alloc_host.py" in msg and "after the payload" not in msg
        r.buf[r.start - 1] = g.guard_byte
        g.check()
        r.buf[r.start + r.nbytes] = 0                # the first byte past the payload (in the padding to 16)
        r.buf[r.start + r.nbytes + 100] = 1
        with pytest.raises(GuardError) as e:
            g.check()
        msg = str(e.value)
        assert "after the payload" in msg and "offset 0 " in msg and "2 byte(s)" in msg and "before the payload" not in msg
        r.buf[r.start + r.nbytes] = g.guard_byte
        r.buf[r.start + r.nbytes + 100] = g.guard_byte
        t.fill_(1.0)                                 # the payload itself is the caller's
        g.check()


def test_a_changed_frozen_input_is_reported():
    with guarded("B", cpu=True) as g:
        x = g.put(np.arange(12, dtype=np.float32).reshape(3, 4))
        y = g.frozen(torch.arange(6, dtype=torch.int32))
        assert x.dtype == torch.float32 and x.shape == (3, 4) and x[2, 3] == 11 and _record(g, x).nbytes == 48
        g.check()
        x[1, 2] = float(np.nextafter(np.float32(6.0), np.float32(7.0)))          # one mantissa bit: byte 0 of element 6
        with pytest.raises(GuardError) as e:
            g.check()
        assert "const input" in str(e.value) and "(3, 4)" in str(e.value) and "1 byte(s), first at byte 24" in str(e.value)
        x[1, 2] = 6.0
        g.check()
        y[5] = 0
        with pytest.raises(GuardError, match="const input"):
            g.check()


def test_everything_is_restored_and_nesting_is_refused():
    orig = (torch.empty, torch.zeros, torch.full, torch.empty_like)
    with guarded("A", cpu=True):
        assert torch.empty is not orig[0]
        with pytest.raises(RuntimeError, match="nest"):
            with guarded("B"):
                pass
        assert torch.empty is not orig[0]            # the refused inner context restored nothing
    assert (torch.empty, torch.zeros, torch.full, torch.empty_like) == orig
    with pytest.raises(KeyError):
        with guarded("A", cpu=True):
            raise KeyError("x")
    assert (torch.empty, torch.zeros, torch.full, torch.empty_like) == orig
    with guarded("B", cpu=True):                     # and it can be entered again
        pass
    with pytest.raises(ValueError):
        guarded("C")


def test_recording_notes_the_entries_called_and_restores_the_handle():
    from disn_amd import _lib
    real = _lib.lib()
    with guarded("A", cpu=True) as g:
        with g.recording() as names:
            assert _lib.lib() is not real
            assert _lib.lib().disn_abi_version() == _lib.ABI_VERSION
            assert _lib.lib().disn_fc_workspace_bytes(4, 1000, 256) == real.disn_fc_workspace_bytes(4, 1000, 256)
            assert _lib.lib().disn_abi_version.restype is real.disn_abi_version.restype
        assert names == ["disn_abi_version", "disn_fc_workspace_bytes"] and _lib.lib() is real
        with pytest.raises(KeyError):
            with g.recording():
                raise KeyError("x")
        assert _lib._LIB is real


# ---------------------------------------------------------------- header coverage --------------------------------
# entries that write no device memory and launch nothing -- the only ones a scenario may leave out
EXEMPT_ALLOWED = re.compile(
    r"^disn_(abi_version|\w+_bytes|\w+_words|\w+_plan|\w*_?layout|param_layout"
    r"|stream_create|stream_destroy|ctx_create|ctx_destroy|ctx_pipeline"
    r"|write_obj|write_obj_normals|write_obj_colours|read_obj_verts|read_obj_mesh|mesh_bvh_build|mesh_bvh_build_order)$")


DECLARED = 162            # the functions the five headers declare today: a floor, so that a parse that misses some fails


def header_entries():
    """the functions of every include/*.h"""
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        out += re.findall(r"\b(disn_\w+)\s*\(", text)
    return out


def covered_in_its_own_file(entry, where):
    """`where` = file::test names a test of tests/ that asserts set(NEW) <= set(called), and that file's NEW lists `entry`"""
    fname, test = where.split("::")
    src = open(os.path.join(ROOT, "tests", fname)).read()
    tree = ast.parse(src)
    new = [n for n in tree.body if isinstance(n, ast.Assign) and [t.id for t in n.targets if isinstance(t, ast.Name)] == ["NEW"]]
    assert len(new) == 1, "%s: one module-level NEW tuple" % fname
    assert entry in ast.literal_eval(new[0].value), "%s: NEW does not list %s" % (fname, entry)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == test]
    assert len(fn) == 1, "%s has no test %s" % (fname, test)
    body = ast.get_source_segment(src, fn[0])
    assert "set(NEW) <= set(called)" in body and "guarded(" in body and ".recording()" in body, where
    gpu = "pytestmark = pytest.mark.gpu" in src or any("gpu" in ast.get_source_segment(src, d) for d in fn[0].decorator_list)
    assert gpu, "%s is not a gpu test" % where


def test_every_header_entry_is_covered_exactly_once():
    import test_gpu_memory_contract as T
    from disn_amd import _lib
    declared = header_entries()
    tables = (_lib.SIGNATURES, _lib.SIGNATURES_SIMPLIFY, _lib.SIGNATURES_COLOUR, _lib.SIGNATURES_SAMPLE,
              _lib.SIGNATURES_SMOOTH)
    bound = [name for t in tables for name in t]
    assert len(bound) == len(set(bound))
    assert len(declared) == len(set(declared)) >= DECLARED and set(declared) == set(bound)
    assert len(glob.glob(os.path.join(ROOT, "include", "*.h"))) == len(tables)       # a sixth header brings its table
    claimed = [e for entries in T.ENTRY_COVERAGE.values() for e in entries]
    listed = claimed + list(T.EXEMPT) + list(T.MESH_MODULE_COVERAGE)
    for entry, where in T.MESH_MODULE_COVERAGE.items():
        assert entry not in _lib.SIGNATURES, "%s belongs to include/disn_amd.h: it needs a scenario" % entry
        covered_in_its_own_file(entry, where)
    twice = sorted({e for e in listed if listed.count(e) > 1})
    assert not twice, "listed more than once: %s" % twice
    assert not sorted(set(listed) - set(declared)), "not in the header: %s" % sorted(set(listed) - set(declared))
    missing = sorted(set(declared) - set(listed))
    assert not missing, "neither run under guards by a scenario nor exempt: %s" % missing
    for name, reason in T.EXEMPT.items():
        assert EXEMPT_ALLOWED.match(name), "%s writes device memory or launches: it needs a scenario" % name
        assert isinstance(reason, str) and len(reason) > 10, name
    assert set(T.ENTRY_COVERAGE) == set(T.SCENARIOS), "a scenario without entries, or entries without a scenario"
    for name, sites in T.FLOAT_ATOMICS.items():      # entries compared by tolerance only: each names its atomic
        assert name in claimed
        for site in sites:
            m = re.match(r"^(disn_amd/csrc/\w+\.hip):(\d+)$", site)
            assert m, site
            line = open(os.path.join(ROOT, m.group(1))).read().split("\n")[int(m.group(2)) - 1]
            assert "atomicAdd" in line or "unsafeAtomicAdd" in line or "atomic_add" in line, (site, line)
