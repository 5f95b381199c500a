"""Ensembles on several contexts, the parts that need no GPU: the blocks Ensemble(devices=...) hands its contexts, the
new prototypes of include/esim.h against the bindings, the arguments Ensemble refuses before it creates a context, and the
descriptor and blob header of esim_merge.h in a program of its own under the host sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

from epidemicsimulator_amd import _lib
from epidemicsimulator_amd import ensemble as ens_mod
from epidemicsimulator_amd.ensemble import Ensemble, split_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("esim_ensemble_merge", "esim_ensemble_save_size", "esim_ensemble_save", "esim_ensemble_load")


@pytest.mark.parametrize("k", range(1, 5))
@pytest.mark.parametrize("n", range(10))
def test_split_members_gives_contiguous_blocks_in_order_the_larger_ones_first(n, k):
    blocks = split_members(n, k)
    assert len(blocks) == k and blocks[0][0] == 0 and blocks[-1][1] == n
    assert all(b[1] == c[0] for b, c in zip(blocks, blocks[1:])), blocks               # contiguous, in order
    sizes = [e - b for b, e in blocks]
    assert all(s >= 0 for s in sizes) and max(sizes) - min(sizes) <= 1, blocks
    assert sizes == sorted(sizes, reverse=True), blocks                                # the larger ones first
    assert [i for b, e in blocks for i in range(b, e)] == list(range(n))


def test_split_members_refuses_no_context_and_a_negative_count():
    for n, k in ((3, 0), (-1, 2)):
        with pytest.raises(ValueError):
            split_members(n, k)


def test_the_header_and_the_bindings_agree():
    header = open(os.path.join(ROOT, "include", "esim.h")).read()
    lib = _lib.load()
    want = {"esim_ensemble_merge": (r"esim_ctx \*dst, esim_ctx \*src", [C.c_void_p, C.c_void_p]),
            "esim_ensemble_save_size": (r"esim_ctx \*ctx, size_t \*bytes", [C.c_void_p, C.POINTER(C.c_size_t)]),
            "esim_ensemble_save": (r"esim_ctx \*ctx, void \*buf, size_t cap", [C.c_void_p, C.c_void_p, C.c_size_t]),
            "esim_ensemble_load": (r"esim_ctx \*ctx, const void \*buf, size_t bytes", [C.c_void_p, C.c_void_p, C.c_size_t])}
    for name in NEW:
        args, argtypes = want[name]
        assert re.search(r"\bint\s+%s\s*\(%s\);" % (name, args), header), name
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    # the constants esim_merge.h repeats are those of the header and of the bindings
    engine = open(os.path.join(ROOT, "epidemicsimulator_amd", "csrc", "esim_merge.h")).read()
    assert "#define MERGE_KEPT_MAX 256u" in engine and re.search(r"#define ESIM_MEMBERS_MAX\s+256\b", header) and _lib.MEMBERS_MAX == 256
    assert "#define MERGE_GROUPS_MAX 1024u" in engine and re.search(r"#define ESIM_MAX_GROUPS\s+1024\b", header) and _lib.MAX_GROUPS == 1024
    assert "one host thread at a time per context, any number of contexts at once" in header
    for doc in ("README.md", "DESIGN.md"):
        assert "ESIM_MERGE_PIECE" in open(os.path.join(ROOT, doc)).read(), doc


def test_ensemble_refuses_bad_devices_before_any_context_is_created(monkeypatch):
    made = []
    monkeypatch.setattr(ens_mod, "Simulator", lambda *a, **k: made.append(a) or (_ for _ in ()).throw(AssertionError("a context was created")))
    for bad in ((), [], (-1,), (0, -2), (0.5,), (True,)):
        with pytest.raises(ValueError):
            Ensemble(object(), devices=bad)
    assert not made


def test_the_descriptor_and_the_blob_header_under_the_host_sanitizers(tmp_path):
    """tests/native/merge_host_check.hip, a program of its own that opens no device: pack and parse of the descriptor for every
    kind, the sizes of hand-computed shapes and every blob the parser must refuse, on buffers of exactly the length passed, built
    with AddressSanitizer and UBSan for the host side.  Where the environment preloads a library of its own into every process,
    the sanitizers' runtime could not come first: the program is then built and run without them, and checks the same."""
    exe = str(tmp_path / "merge_host_check")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17"] + sanitize + [
           "-I", os.path.join(ROOT, "epidemicsimulator_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "merge_host_check.hip")]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-2000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and "merge_host_check: ok" in ran.stdout, (ran.returncode, ran.stdout[-500:], ran.stderr[-2000:])
