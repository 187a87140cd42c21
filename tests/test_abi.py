"""The C-ABI library loads and exports every function include/*.h declares; the device
surface refuses cleanly (ENODEV) where there is no MI355X.  No compute on a GPU here."""
import ctypes as C
import glob
import os
import re

import pytest

import uvhttp_amd as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    names = set()
    for h in glob.glob(os.path.join(REPO, "include", "*.h")):
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        for m in re.finditer(r"^[A-Za-z_][\w\s\*]*?\b(uvhttp_\w+)\s*\(", src, flags=re.M):
            if "typedef" in src[src.rfind("\n", 0, m.start()) + 1:m.end()]:
                continue
            names.add(m.group(1))
    return sorted(names)


def test_every_declared_symbol_is_exported():
    names = _declared_functions()
    assert len(names) >= 19, names
    L = C.CDLL(U.LIB_PATH)
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_version_string():
    assert b"gfx950" in U.lib().uvhttp_ws_amd_version()


def test_gfx950_code_object_present():
    """The library carries a gfx950 code object (offload bundle)."""
    blob = open(U.LIB_PATH, "rb").read()
    assert b"gfx950" in blob


def test_no_gpu_means_enodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    assert U.lib().uvhttp_ws_gpu_engine_create(0, C.byref(h)) == -2
    assert U.lib().uvhttp_tls_gpu_engine_create(0, C.byref(h)) == -2
    with pytest.raises(U.GpuError):
        U.GpuEngine(0)
    with pytest.raises(U.GpuError):
        U.TlsEngine(0)


def test_product_does_not_reference_oracle():
    """The product library and package never load the oracle (no CPU fallback path), nor the
    reference build beside it (oracle/_ref/libws_ref.so and its driver's ws_ref_* calls)."""
    for p in glob.glob(os.path.join(REPO, "uvhttp_amd", "**", "*"), recursive=True):
        if os.path.isfile(p) and p.endswith((".py", ".c", ".cpp", ".hip", ".h")):
            txt = open(p).read()
            assert "libws_oracle" not in txt and "import _oracle" not in txt, p
            assert "oracle/_ref" not in txt and "libws_ref" not in txt and "ws_ref_" not in txt, p
            assert "import _reference" not in txt, p
    for path in (U.LIB_PATH, U.TESTHOOKS_LIB_PATH):
        blob = open(path, "rb").read()
        assert b"libws_oracle" not in blob and b"oracle_" not in blob, path
        assert b"oracle/_ref" not in blob and b"libws_ref" not in blob and b"ws_ref_" not in blob, path


def test_fault_injection_only_in_the_test_build():
    """The batcher's fault-injection variable is read only by the test build
    (libuvhttp_ws_amd_testhooks.so, -DUVWS_TEST_HOOKS); the product library has no such hook."""
    assert b"UVHTTP_WS_BATCHER_FAIL_EVERY" not in open(U.LIB_PATH, "rb").read()
    assert b"UVHTTP_WS_BATCHER_FAIL_EVERY" in open(U.TESTHOOKS_LIB_PATH, "rb").read()


# switches of decode variants that were measured slower or even and deleted with their code
REMOVED_KNOBS = ("UVHTTP_WS_STORE_POLICY", "UVHTTP_WS_PLAN_TICKET", "UVHTTP_WS_STREAM_NT",
                 "UVHTTP_WS_WALK_NT_LOAD", "UVHTTP_WS_COMPACT_RECS", "UVHTTP_WS_FUSED_AUX",
                 "UVHTTP_WS_FUSED_TILE", "UVHTTP_WS_FIXUP_BLOCKS")


def test_product_library_reads_no_environment():
    """the switches that force a path (UVHTTP_WS_WALK, UVHTTP_WS_FUSED, ...)
    are compiled only into the experiment build (-DUVWS_EXPERIMENTS); the product library names
    none of them and imports no getenv at all.  The Python mirror routes an engine created while
    a switch is set to the experiment build.  Switches of variants that were deleted — among
    them UVHTTP_WS_PLAN_TICKET=0, whose blockIdx-ordered workgroups relied on in-order dispatch
    (k_plan and the fused stream walk always take tickets now) — are in neither library."""
    prod = open(U.LIB_PATH, "rb").read()
    exp = open(U.TESTHOOKS_LIB_PATH, "rb").read()
    for k in U.EXPERIMENT_KNOBS:
        assert k.encode() not in prod, k
    for k in ("UVHTTP_WS_WALK", "UVHTTP_WS_FUSED", "UVHTTP_WS_COMPACT", "UVHTTP_TLS_CRYPT_GRID"):
        assert k.encode() in exp, k
    for k in REMOVED_KNOBS:
        assert k.encode() not in prod and k.encode() not in exp, k
    import subprocess
    syms = subprocess.run(["nm", "-D", "--undefined-only", U.LIB_PATH], capture_output=True,
                          text=True).stdout
    assert " getenv" not in syms and "secure_getenv" not in syms


def test_knob_routes_to_experiment_build(monkeypatch):
    monkeypatch.delenv("UVHTTP_WS_COMPACT", raising=False)
    for k in U.EXPERIMENT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert U.default_library() is U.lib()
    monkeypatch.setenv("UVHTTP_WS_WALK", "lane")
    assert U.default_library() is U.test_hooks_library()
