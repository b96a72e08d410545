#!/usr/bin/env python3
"""The host half of the library under AddressSanitizer and UndefinedBehaviorSanitizer, in a stand-alone program.

    python tools/abi_sanitize.py [--verbose]

1. writes a C++ program with its own main: every mutated call of the argument sweep (tests/abi_table.py, the calls of
   tests/test_abi_errors_host.py) as a literal call with its expected status, then the host-only entries on real inputs
   -- a corpus of malformed Wavefront files for the readers, degenerate meshes for the BVH builder, the component
   labelling and the writers, CRC-32C at every alignment, the weight equalisation on all its tensors;
2. compiles the library's sources with their own flags of disn_amd/csrc/build.py plus
   -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined (the device code is untouched),
   objects cached by digest under disn_amd/csrc/build/san/ as build.py caches its own;
3. links program and objects with clang++ -fsanitize=address,undefined (no shared library, nothing preloaded) and runs
   it with the device hidden: no call of the program may reach a launch, and none needs a device.

Exit status 0: every call returned what the table expects and neither sanitizer reported anything."""
from __future__ import annotations

import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import abi_table as T  # noqa: E402
from disn_amd.csrc import build as B  # noqa: E402

OUT = os.path.join(B.HERE, "build", "san")
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
SAN_COMPILE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
SAN_LINK = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CTYPES = {"f": "float", "d": "double", "i": "int32_t", "q": "int64_t", "Q": "uint64_t", "B": "uint8_t"}
STRUCTS = {"vgg": "disn_vgg_weights_t", "mlp": "disn_mlp_weights_t", "cam": "disn_cam_weights_t", "eq": "disn_eq_weights_t",
           "layout": "disn_param_layout_t", "cam_layout": "disn_cam_param_layout_t"}


# ---------------------------------------------------------------- the sweep as literal calls ----------------------
def _lit(v, cls):
    if cls in ("float", "double"):
        return repr(float(v)) + ("f" if cls == "float" else "")
    if cls == "int64_t":
        return "(int64_t)%dLL" % v if v != -2 ** 63 else "INT64_MIN"
    if cls == "size_t":
        return "(size_t)%dULL" % v
    return "%d" % v if cls == "int" else "(uint32_t)%du" % v


def _need(tok, protos):
    q = protos[tok[1]]
    args = []
    for a, (ctype, _) in zip(tok[2], q.params):
        args.append(_lit(a, T.c_class(ctype)) if not isinstance(a, (tuple, list)) else _need(a, protos))
    return "%s(%s)" % (tok[1], ", ".join(args))


def render_call(call, protos, n):
    """one block: the host objects of the call, the call, the check of its status"""
    proto = protos[call.entry]
    decl, args = [], []
    for k, (tok, (ctype, pname)) in enumerate(zip(call.args, proto.params)):
        cls = T.c_class(ctype)
        if not isinstance(tok, (tuple, list)):
            args.append(_lit(tok, cls))
            continue
        kind = tok[0]
        if kind == "null":
            args.append("nullptr")
        elif kind == "fake":
            args.append("(%s)FAKE" % ctype)
        elif kind == "host":
            decl.append("%s h%d[] = {%s};" % (CTYPES[tok[1]], k, ", ".join(repr(v) for v in tok[2])))
            args.append("(%s)h%d" % (ctype, k))
        elif kind == "need":
            args.append(_need(tok, protos) + (" + %d" % tok[3] if tok[3] else ""))
        elif kind == "big":
            args.append("((size_t)1 << 62)")
        else:
            assert kind == "obj", tok
            o = tok[1]
            if o == "path":
                args.append("SWEEP_PATH")
            elif o in STRUCTS:
                decl.append("%s o%d; fill(&o%d, sizeof o%d);" % (STRUCTS[o], k, k, k))
                if o in ("vgg", "eq"):
                    decl.append("o%d.num_classes = 1024;" % k)
                if o == "vgg":
                    decl.append("o%d.strict_forms = 0;" % k)
                args.append("&o%d" % k)
            elif o == "taps5":
                decl.append("float* o%d[5] = {(float*)FAKE, (float*)FAKE, (float*)FAKE, (float*)FAKE, (float*)FAKE};" % k)
                args.append("(%s)o%d" % (ctype, k))
            elif o == "box6":
                decl.append("double o%d[6] = {-1, -1, -1, 1, 1, 1};" % k)
                args.append("o%d" % k)
            elif o == "k9":
                decl.append("float o%d[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};" % k)
                args.append("o%d" % k)
            else:
                assert o == "slot" and ctype.endswith("*"), (call.entry, pname, tok)
                base = ctype[:-1].replace("const ", "")
                decl.append("%s o%d = 0;" % (base, k))
                args.append("&o%d" % k)
    label = "%s / %s" % (call.entry, call.label)
    invoke = "%s(%s)" % (call.entry, ", ".join(args))
    kind = call.expect[0]
    guard = ""
    if kind in ("eq_if_need", "neg_if_need"):
        i = [k for k, a in enumerate(call.args) if isinstance(a, (tuple, list)) and a[0] == "need"][0]
        guard = "if (%s > 0) " % _need(call.args[i], protos)
    if kind in ("eq", "eq_if_need"):
        check = "expect_eq(\"%s\", (long long)%s, %d);" % (label, invoke, call.expect[1])
    elif kind in ("neg", "neg_if_need"):
        check = "expect_neg(\"%s\", (long long)%s);" % (label, invoke)
    elif kind == "zero":
        check = "expect_eq(\"%s\", (long long)%s, 0);" % (label, invoke)
    elif kind == "pos":
        check = "expect_pos(\"%s\", (long long)%s);" % (label, invoke)
    else:
        assert kind == "zero_or_ge", kind
        check = "expect_zero_or_ge(\"%s\", %s, %s);" % (label, invoke, _need(call.expect[1], protos))
    return "  %s{ %s\n    %s }\n" % (guard, " ".join(decl), check)


PRELUDE = r'''// generated by tools/abi_sanitize.py -- do not edit
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "disn_amd.h"
#include "disn_amd_simplify.h"
#include "disn_amd_colour.h"
#include "disn_amd_sample.h"
#include "disn_amd_smooth.h"

static void* const FAKE = (void*)0x10000;     // a device pointer no host path may dereference
static int g_bad = 0, g_calls = 0;
static const char* SWEEP_PATH = nullptr;
static void fill(void* p, size_t n) {          // every pointer field of a weight struct: the fake device pointer
  for (size_t i = 0; i + sizeof(void*) <= n; i += sizeof(void*)) std::memcpy((char*)p + i, &FAKE, sizeof(void*));
}
static void bad(const char* what, long long r, const char* want) {
  std::printf("FAIL %s returned %lld: expected %s\n", what, r, want);
  ++g_bad;
}
static void expect_eq(const char* what, long long r, long long v) {
  ++g_calls;
  if (r != v) bad(what, r, std::to_string(v).c_str());
}
static void expect_neg(const char* what, long long r) {
  ++g_calls;
  if (r >= 0) bad(what, r, "a negative status");
}
static void expect_pos(const char* what, long long r) {
  ++g_calls;
  if (r <= 0) bad(what, r, "> 0");
}
static void expect_zero_or_ge(const char* what, size_t r, size_t least) {
  ++g_calls;
  if (r != 0 && r < least) bad(what, (long long)r, "0 or at least the CASE's");
}
'''

SECTION2 = r'''
// ---- the host-only entries on real inputs ---------------------------------------------------------------------
static void read_one(const std::string& path) {
  const int64_t nv = disn_read_obj_verts(path.c_str(), nullptr, 0);
  ++g_calls;
  if (nv > 0) {
    std::vector<float> v(3 * nv);
    if (disn_read_obj_verts(path.c_str(), v.data(), nv) != nv) bad(path.c_str(), nv, "the same count on the second read");
    std::vector<float> one(3);
    disn_read_obj_verts(path.c_str(), one.data(), 1);            // a capacity below the count: only the first row
  }
  int64_t counts[2] = {-7, -7};
  const int rc = disn_read_obj_mesh(path.c_str(), nullptr, 0, nullptr, 0, counts);
  ++g_calls;
  if (rc != 0 && rc != DISN_E_ARG && rc != DISN_E_SHAPE) bad(path.c_str(), rc, "0, DISN_E_ARG or DISN_E_SHAPE");
  if (rc == 0) {
    std::vector<float> v(3 * counts[0] + 3);
    std::vector<int32_t> f(3 * counts[1] + 3);
    int64_t again[2];
    if (disn_read_obj_mesh(path.c_str(), v.data(), counts[0], f.data(), counts[1], again) != 0 || again[0] != counts[0] ||
        again[1] != counts[1])
      bad(path.c_str(), again[1], "the same counts on the second read");
    for (int64_t i = 0; i < 3 * counts[1]; ++i)
      if (f[i] < 0 || f[i] >= counts[0]) bad(path.c_str(), f[i], "an index inside [0, nv)");
    disn_read_obj_mesh(path.c_str(), v.data(), counts[0] > 0 ? 1 : 0, f.data(), counts[1] > 0 ? 1 : 0, again);   // small caps
  }
}

static void mesh_one(const char* what, const std::vector<float>& v, const std::vector<int32_t>& f, const std::string& dir) {
  const int64_t nv = (int64_t)v.size() / 3, nf = (int64_t)f.size() / 3;
  const size_t need = disn_mesh_bvh_bytes(nf);
  std::vector<char> bvh(need ? need : 1), bvh2(need ? need : 1);
  std::vector<int32_t> order(nf ? nf : 1);
  const int r1 = disn_mesh_bvh_build(v.data(), nv, f.data(), nf, bvh.data(), need);
  const int r2 = disn_mesh_bvh_build_order(v.data(), nv, f.data(), nf, bvh2.data(), need, order.data());
  g_calls += 2;
  if (r1 != r2 || r1 > 0) bad(what, r1, "one status <= 0 from both builders");
  if (r1 == 0 && std::memcmp(bvh.data(), bvh2.data(), need)) bad(what, 0, "the same image from both builders");
  std::vector<int32_t> labels(nf ? nf : 1);
  for (int conn = 0; conn < 2; ++conn) {
    int64_t ncomp = -1;
    const int rc = disn_mesh_components(f.data(), nf, nv, conn, labels.data(), &ncomp);
    ++g_calls;
    if (rc > 0) bad(what, rc, "a status <= 0 from disn_mesh_components");
  }
  std::vector<float> nrm(v.size(), 0.5f);
  std::vector<uint8_t> col(v.size(), 128);
  const std::string p = dir + "/out.obj";
  bool in_range = true;
  for (int32_t i : f) in_range = in_range && i >= 0 && i < nv;
  if (in_range) {                                              // the writers print what they are given
    if (disn_write_obj(p.c_str(), v.data(), nv, f.data(), nf) != 0) bad(what, -1, "0 from disn_write_obj");
    read_one(p);
    if (disn_write_obj_normals(p.c_str(), v.data(), nv, nrm.data(), f.data(), nf) != 0) bad(what, -1, "0 from disn_write_obj_normals");
    read_one(p);
    if (disn_write_obj_colours(p.c_str(), v.data(), nv, col.data(), nrm.data(), f.data(), nf) != 0) bad(what, -1, "0 from disn_write_obj_colours");
    read_one(p);
    if (disn_write_obj_colours(p.c_str(), v.data(), nv, col.data(), nullptr, f.data(), nf) != 0) bad(what, -1, "0 without normals");
    read_one(p);
    g_calls += 4;
  }
}

static void equalise() {
  static const int cin[13] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
  static const int cout[13] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
  static const int mcout[6] = {64, 256, 512, 512, 256, 1};
  std::vector<std::vector<float>> keep;
  unsigned s = 12345u;
  auto tensor = [&](size_t n) {
    keep.emplace_back(n);
    for (float& x : keep.back()) {
      s = s * 1664525u + 1013904223u;
      x = ((int)(s >> 8) % 2001 - 1000) * 1e-3f;
    }
    return keep.back().data();
  };
  disn_eq_weights_t w;
  std::memset(&w, 0, sizeof w);
  w.num_classes = 1024;
  for (int i = 0; i < 13; ++i) {
    w.conv_w[i] = tensor((size_t)9 * cin[i] * cout[i]);
    w.conv_b[i] = tensor(cout[i]);
  }
  w.fc6_w = nullptr;                                           // "NULL = not present"
  for (int st = 0; st < 2; ++st) {
    const int mcin[6] = {3, 64, 256, st == 0 ? 512 + 1024 : 1984, 512, 256};
    for (int l = 0; l < 6; ++l) {
      w.mlp_w[st][l] = tensor((size_t)mcin[l] * mcout[l]);
      w.mlp_b[st][l] = tensor(mcout[l]);
    }
  }
  keep[2][7] = 0.f;                                            // a zero entry, a dead column, a huge and a denormal one
  for (int r = 0; r < 9 * 64; ++r) keep[2][(size_t)r * 64 + 5] = 0.f;
  keep[4][11] = 3.0e38f;
  keep[6][13] = 1.0e-42f;
  std::vector<float> tap(1472), span(23);
  int rc = disn_equalise_weights(&w, tap.data(), span.data());
  if (rc != 0) bad("disn_equalise_weights", rc, "0");
  rc = disn_equalise_weights(&w, tap.data(), nullptr);         // a second pass, without the spans
  if (rc != 0) bad("disn_equalise_weights (second pass)", rc, "0");
  g_calls += 2;
}

static void crc() {
  std::vector<unsigned char> buf(4099);
  for (size_t i = 0; i < buf.size(); ++i) buf[i] = (unsigned char)(i * 131u + 7u);
  if (disn_crc32c("123456789", 9, 0) != 0xE3069283u) bad("disn_crc32c", 0, "the CRC-32C check value");
  for (size_t off = 0; off < 9; ++off)
    for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)8, (size_t)63, (size_t)4090}) {
      const uint32_t whole = disn_crc32c(buf.data() + off, n, 0);
      const uint32_t head = disn_crc32c(buf.data() + off, n / 3, 0);
      if (disn_crc32c(buf.data() + off + n / 3, n - n / 3, head) != whole) bad("disn_crc32c", (long long)n, "a continued sum equal to the whole");
      ++g_calls;
    }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  const int nfiles = std::atoi(argv[2]);
  const std::string sweep_path = dir + "/sweep.obj";
  SWEEP_PATH = sweep_path.c_str();
  sweep();
  for (int i = 0; i < nfiles; ++i) read_one(dir + "/corpus_" + std::to_string(i) + ".obj");
  read_one(dir + "/does_not_exist.obj");
  const float nan = std::numeric_limits<float>::quiet_NaN();
  mesh_one("all vertices equal", {1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3}, {0, 1, 2, 1, 2, 3, 0, 0, 0}, dir);
  mesh_one("a NaN vertex", {0, 0, 0, 1, 0, 0, nan, 1, 0, 0, 0, 1}, {0, 1, 2, 0, 1, 3, 1, 2, 3}, dir);
  mesh_one("an index equal to nv", {0, 0, 0, 1, 0, 0, 0, 1, 0}, {0, 1, 2, 0, 1, 3}, dir);
  mesh_one("a negative index", {0, 0, 0, 1, 0, 0, 0, 1, 0}, {0, 1, -1}, dir);
  mesh_one("nf = 1", {0, 0, 0, 1, 0, 0, 0, 1, 0}, {0, 1, 2}, dir);
  mesh_one("infinite and huge coordinates", {0, 0, 0, 3e38f, -3e38f, 0, 0, INFINITY, 0, 1, 1, 1}, {0, 1, 2, 1, 2, 3}, dir);
  {
    std::vector<float> v;
    std::vector<int32_t> f;
    for (int i = 0; i < 300; ++i) {                            // a strip: more than one BVH leaf, one component
      v.insert(v.end(), {(float)i, (float)(i & 1), 0.f});
      if (i >= 2) f.insert(f.end(), {i - 2, i - 1, i});
    }
    mesh_one("a strip of 298 triangles", v, f, dir);
  }
  crc();
  equalise();
  std::printf("%s: %d calls, %d wrong\n", g_bad ? "FAILED" : "ok", g_calls, g_bad);
  return g_bad ? 1 : 0;
}
'''

# name, bytes: what a reader may meet.  The readers return a count or DISN_E_ARG; they never read past the file.
CORPUS = [
    ("empty", b""),
    ("v alone", b"v\n"),
    ("two coordinates", b"v 1 2\n"),
    ("coordinates continued on the next line", b"v 1 2\n3\nv 4 5 6\n"),
    ("f with two indices", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n"),
    ("index 0", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n"),
    ("negative out of range", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n"),
    ("negative in range", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -3\n"),
    ("a 20-digit index", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 99999999999999999999\n"),
    ("an index past int64", b"v 0 0 0\nf 1 1 " + b"9" * 400 + b"\n"),
    ("v/vt/vn forms", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\nf 1//1 2//1 4//1\nf 1/1 2/1 3/1\n"),
    ("a slash with nothing before it", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf /1 2 3\nf 1/ 2/ 3/\n"),
    ("CRLF", b"v 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nf 1 2 3\r\n"),
    ("tabs", b"v\t0\t0\t0\nv\t1\t0\t0\nv\t0\t1\t0\nf\t1\t2\t3\n"),
    ("no final newline", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3"),
    ("an embedded NUL", b"v 0 0 0\nv 1 \x00 0 0\nv 0 1 0\nf 1 2 3\n"),
    ("1e400 nan inf", b"v 1e400 nan inf\nv -1e400 -nan -inf\nv 1e-400 0x1p3 .5\nf 1 2 3\n"),
    ("polygons", b"v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv .5 2 0\nf 1 2 3 4 5\nf 1 2 3 4\n"),
    ("a very long line", b"v 0 0 0\nv 1 0 0\nv 0 1 0\n# " + b"x" * 70000 + b"\nf 1 2 3 " + b" " * 70000 + b"\n"),
    ("a face before its vertices", b"f 1 2 3\nv 0 0 0\nv 1 0 0\nv 0 1 0\n"),
    ("only a keyword prefix", b"vx 1 2 3\nfoo 1 2 3\nv\nf\nf \n"),
    ("binary noise", bytes((i * 197 + 13) & 0xFF for i in range(5000))),
]


def write_program(verbose=False):
    os.makedirs(OUT, exist_ok=True)
    protos = T.parse_headers()
    T.check_against_binding(protos)
    T.check_complete(protos)
    calls = list(T.all_calls(protos))
    chunks, body = [], []
    for n, c in enumerate(calls):
        body.append(render_call(c, protos, n))
        if len(body) == 150 or n == len(calls) - 1:             # many small functions: the compiler's stack and time
            chunks.append("static void sweep_%d() {\n%s}\n" % (len(chunks), "".join(body)))
            body = []
    src = PRELUDE + "".join(chunks) + "static void sweep() {\n%s}\n" % "".join("  sweep_%d();\n" % i for i in range(len(chunks)))
    src += SECTION2
    path = os.path.join(OUT, "abi_sanitize_main.cpp")
    if not os.path.exists(path) or open(path).read() != src:
        with open(path, "w") as f:
            f.write(src)
    for i, (_, data) in enumerate(CORPUS):
        with open(os.path.join(OUT, "corpus_%d.obj" % i), "wb") as f:
            f.write(data)
    if verbose:
        print("%d sweep calls, %d corpus files -> %s" % (len(calls), len(CORPUS), path))
    return path, len(calls)


def compile_objects(verbose=False):
    """the library's sources under the sanitizers, cached by the digest of source, headers and flags"""
    hdrs = [h if os.path.isabs(h) else os.path.join(B.HERE, h) for h in B.HEADERS]
    objs, jobs = [], []
    for src, flags in B.SOURCES.items():
        sp = os.path.join(B.HERE, src)
        if not os.path.exists(sp):
            continue
        full = B.COMMON + flags + SAN_COMPILE
        obj = os.path.join(OUT, "%s.%s.o" % (src, B._digest([sp] + hdrs, " ".join(full))))
        objs.append(obj)
        if not os.path.exists(obj):
            jobs.append((sp, obj, full))

    def one(job):
        sp, obj, full = job
        cmd = [B.HIPCC] + full + ["-c", sp, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (sp, r.stdout, r.stderr))

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(one, jobs))
    for fn in os.listdir(OUT):                                  # objects of earlier source states
        if fn.endswith(".o") and os.path.join(OUT, fn) not in objs and not fn.startswith("abi_sanitize_main"):
            os.remove(os.path.join(OUT, fn))
    return objs, len(jobs)


def link(main_cpp, objs, verbose=False):
    exe = os.path.join(OUT, "abi_sanitize")
    stamp = os.path.join(OUT, "link.stamp")
    want = B._digest([main_cpp] + objs, " ".join(SAN_LINK))
    if os.path.exists(exe) and os.path.exists(stamp) and open(stamp).read() == want:
        return exe
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(B.HIPCC)), "lib")
    cmd = [CLANGXX, "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include")] + SAN_LINK + [main_cpp] + objs + \
          ["-L" + rocm_lib, "-lamdhip64", "-Wl,-rpath," + rocm_lib, "-o", exe]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:]))
    with open(stamp, "w") as f:
        f.write(want)
    return exe


def run(exe):
    env = dict(os.environ)                                      # as it is: the program needs nothing preloaded
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="",
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, OUT, str(len(CORPUS))], capture_output=True, text=True, env=env, timeout=900)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    verbose = "--verbose" in argv or "-v" in argv
    t0 = time.time()
    main_cpp, ncalls = write_program(verbose)
    objs, built = compile_objects(verbose)
    t1 = time.time()
    exe = link(main_cpp, objs, verbose)
    t2 = time.time()
    r = run(exe)
    t3 = time.time()
    print(r.stdout[-4000:], end="")
    if r.returncode != 0:
        print(r.stderr[-6000:], file=sys.stderr)
    print("abi_sanitize: %d objects compiled in %.1f s, link %.1f s, run %.1f s, exit status %d"
          % (built, t1 - t0, t2 - t1, t3 - t2, r.returncode))
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
