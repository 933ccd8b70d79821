"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports
every symbol include/qmg_hip.h declares.  No compute call is made (there is no GPU here)."""
import ctypes
import importlib
import os
import re

import pytest

qmg = importlib.import_module("quantum-mg_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    qmg.build()
    return qmg.lib()


def header_symbols():
    text = open(os.path.join(ROOT, "include", "qmg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(qmg_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert header_symbols() == sorted(qmg.ABI_SYMBOLS)


def test_library_exports_every_declared_symbol(so):
    for name in header_symbols():
        assert hasattr(so, name), "libqmg_hip.so does not export %s" % name


def test_status_strings_and_version(so):
    assert so.qmg_status_string(0) == b"success"
    assert b"gfx950" in so.qmg_version()
    assert so.qmg_status_string(3) == b"unsupported"


def test_tuning_keys_retained_and_retired(so):
    """qmg_set_tuning only sets host globals: every kept key takes its default, the retired A/B keys are unknown keys."""
    success, invalid = 0, 1
    defaults = {"stencil_pair": 2, "pair_prefetch": 1, "stencil_site": 3, "stencil_mfma": 1, "blas_nt_mb": 256,
                "wilson_pair": 2, "setup_fused": 1, "reduce_spin": 1, "malloc_poison": 0}
    for key, value in defaults.items():
        assert so.qmg_set_tuning(key.encode(), value) == success, key
    retired = ("stencil_nt", "stencil_ablate", "stencil_rows", "gen_sites", "gen32", "mfma_vl", "mfma_pair8",
               "site_block", "site_gy", "site_generic", "xfer_tile", "xfer_pack", "xfer_mfma")
    for key in retired:
        for value in (0, 1, 2):
            assert so.qmg_set_tuning(key.encode(), value) == invalid, (key, value)
    for value in (-1, 1, 3, 4, 8, 10):
        assert so.qmg_set_tuning(b"stencil_pair", value) == invalid, value
    assert so.qmg_set_tuning(b"stencil_pair", 0) == success
    assert so.qmg_set_tuning(b"stencil_pair", 2) == success


def test_desc_struct_layout_matches_header():
    # int Lx,Ly,nc (+pad) ; 2 pointers ; 6 doubles
    assert ctypes.sizeof(qmg.StencilDesc) == 16 + 16 + 48
    assert qmg.StencilDesc.clover.offset == 16 and qmg.StencilDesc.shift.offset == 32


def test_library_has_gfx950_code_object():
    data = open(qmg.SO_PATH, "rb").read()
    assert b"gfx950" in data


def test_product_does_not_reference_the_oracle():
    """The product path must not include, link or import anything under oracle/."""
    pkg = os.path.join(ROOT, "quantum-mg_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".hip", ".h", ".hpp", ".cpp", ".py", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "qmg_oracle" not in text and "oracle_lib" not in text, os.path.join(dirpath, f)
    out = os.popen("ldd %s" % qmg.SO_PATH).read()
    assert "oracle" not in out
