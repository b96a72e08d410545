"""tools/abi_sanitize.py: the library's host code under AddressSanitizer and UndefinedBehaviorSanitizer, in a stand-alone
program with its own main -- every call of the argument sweep (tests/abi_table.py) as a literal call, then the host-only
entries on a corpus of malformed .obj files and degenerate meshes.  The program runs with the device hidden and nothing
preloaded; the objects are cached by digest, so only the first run after a source change compiles."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_is_clean_under_asan_and_ubsan():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_sanitize.py")], capture_output=True, text=True,
                       cwd=ROOT, timeout=1800)
    tail = r.stdout[-3000:] + r.stderr[-6000:]
    assert r.returncode == 0, tail
    assert "runtime error" not in tail and "AddressSanitizer" not in tail, tail
    lines = [l for l in r.stdout.splitlines() if l.startswith("ok: ")]
    assert len(lines) == 1, tail
    calls = int(lines[0].split()[1])
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import abi_table as T
    assert calls > len(list(T.all_calls())) - 8        # the sweep (less the calls a CASE without a workspace skips) and more


def test_the_generated_program_holds_every_sweep_call_and_the_corpus():
    sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))]
    import abi_sanitize as S
    import abi_table as T
    path, ncalls = S.write_program()
    src = open(path).read()
    calls = list(T.all_calls())
    assert ncalls == len(calls)
    for c in calls:
        assert '"%s / %s"' % (c.entry, c.label) in src, (c.entry, c.label)
    for entry in ("disn_read_obj_mesh", "disn_read_obj_verts", "disn_mesh_bvh_build", "disn_mesh_bvh_build_order",
                  "disn_mesh_components", "disn_write_obj", "disn_write_obj_normals", "disn_write_obj_colours",
                  "disn_crc32c", "disn_equalise_weights"):
        assert entry + "(" in src.split("the host-only entries on real inputs")[1], entry
    names = [n for n, _ in S.CORPUS]
    for want in ("empty", "v alone", "two coordinates", "coordinates continued on the next line", "f with two indices",
                 "index 0", "negative out of range", "a 20-digit index", "v/vt/vn forms", "CRLF", "tabs", "no final newline",
                 "an embedded NUL", "1e400 nan inf", "polygons"):
        assert want in names, want
    assert len(names) >= 19 and all(os.path.exists(os.path.join(S.OUT, "corpus_%d.obj" % i)) for i in range(len(names)))
