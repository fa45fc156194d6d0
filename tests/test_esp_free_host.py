"""The matrix-free route of GreedyESP without a GPU: the NumPy restatement of the history recurrence
(tests/esp_free_restatement.py) against itself in two precisions and against the dense restatement, and the C surface."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import esp_free_restatement as F
import esp_restatement as R
from mac_amd import _lib

LARGE_SEED = 2      # n = 40 000, m = 20 000, K = 300: smallest relative margin 1.8e-5
LARGE_K = 300


def test_large_case_float64_and_longdouble_agree():
    """The reference error of the large case: the recurrence in float64 against the same recurrence in np.longdouble.  The
    printed figure is what tests/test_esp_free_gpu.py derives its gain tolerance from (it recomputes it)."""
    g = F.large_case(LARGE_SEED)
    o64, g64, m64 = F.greedy(*g, LARGE_K)
    old, gld, _ = F.greedy(*g, LARGE_K, dtype=np.longdouble)
    print("smallest relative margin %.3g" % m64.min())
    assert m64.min() > 1e-6                     # the sequence is pinned
    assert np.array_equal(o64, old)
    d = float(np.max(np.abs(g64 - gld) / np.abs(gld)))
    print("float64 vs longdouble, gains: largest relative difference %.3g" % d)
    assert len(g64) == LARGE_K and g64[0] > 1e4 and 50 < g64[-1] < 1e3      # gains fall from ~7e4 to ~140
    if np.finfo(np.longdouble).eps < 1e-18:     # (where longdouble is wider than float64 the difference is float64's error)
        assert d < 1e-11


def test_history_recurrence_matches_the_dense_restatement():
    rng = np.random.default_rng(5)
    n = 400
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    iu, ju = np.triu_indices(n, 2)
    pick = rng.random(len(iu)) < 0.01
    ci, cj, cw = iu[pick], ju[pick], rng.uniform(0.5, 2.0, int(pick.sum()))
    ci = np.concatenate([ci, [0, 7, 9]]); cj = np.concatenate([cj, [350, 0, 9]]); cw = np.concatenate([cw, [1.1, 0.9, 2.0]])
    K = 150
    od, gd, md = R.greedy(n, fi, fj, fw, ci, cj, cw, K)
    of, gf, mf = F.greedy(n, fi, fj, fw, ci, cj, cw, K)
    assert md.min() > 1e-8
    assert np.array_equal(od, of)
    assert np.all(np.abs(gd - gf) <= 1e-10 * np.abs(gd))
    assert np.allclose(md, mf, rtol=1e-5, atol=0)


def test_restatement_rejects_a_fixed_graph_that_is_not_the_chain():
    with pytest.raises(AssertionError):
        F.greedy(4, [0, 1, 1], [1, 2, 3], [1.0, 1.0, 1.0], [0], [3], [1.0], 1)
    with pytest.raises(AssertionError):
        F.greedy(4, [0, 1], [1, 2], [1.0, 1.0], [0], [3], [1.0], 1)


def test_header_and_library_carry_the_matrix_free_flag():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 10
    assert int(re.search(r"#define MACHIP_ESP_MATRIX_FREE (\d+)", hdr).group(1)) == 2 == _lib.ESP_MATRIX_FREE
    assert int(re.search(r"#define MACHIP_ESP_DENSE_INVERSE (\d+)", hdr).group(1)) == 1 == _lib.ESP_DENSE_INVERSE
    lib = _lib.load()
    assert lib.machip_version() >= 10
    assert "esp_free_split" in _lib.option_names()
    for name in ("machip_esp_create", "machip_esp_select", "machip_esp_weighted_resistances", "machip_esp_info"):
        assert re.search(r"\b%s\(" % name, hdr) and hasattr(lib, name), name


def test_matrix_free_is_keyword_only_and_off_by_default():
    from mac_amd.solvers import GreedyESP
    for f in (GreedyESP.__init__, _lib.Esp.__init__):
        p = inspect.signature(f).parameters["matrix_free"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_argument_errors_are_decided_before_a_device_is_needed():
    """The flag's argument checks come before the device is touched: they answer the same with or without a GPU."""
    import ctypes as C
    lib = _lib.load()
    i32, f64, p_i32, p_f64 = _lib.i32, _lib.f64, _lib.p_i32, _lib.p_f64

    def create(fi, fj, fw, flags, n=4, fold=0):
        fi, fj, fw = i32(fi), i32(fj), f64(fw)
        ci, cj, cw = i32([0]), i32([3]), f64([1.0])
        h = C.c_void_p()
        st = lib.machip_esp_create(0, n, len(fw), p_i32(fi), p_i32(fj), p_f64(fw), 1, p_i32(ci), p_i32(cj), p_f64(cw), fold, flags,
                                   C.byref(h))
        if st == _lib.OK:
            lib.machip_esp_destroy(h)
        return st, _lib.last_error()

    st, msg = create([0, 1, 2], [1, 2, 3], [1.0, 1.0, 1.0], _lib.ESP_MATRIX_FREE | _lib.ESP_DENSE_INVERSE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_DENSE_INVERSE" in msg
    st, msg = create([0, 1, 1], [1, 2, 3], [1.0, 1.0, 1.0], _lib.ESP_MATRIX_FREE)          # a star-ish tree: connected, not the chain
    assert st == _lib.BAD_ARG and "chain" in msg
    st, msg = create([0, 1, 2], [1, 2, 3], [1.0, 1.0, 1.0], 4)
    assert st == _lib.BAD_ARG and "unknown flags" in msg
    st, msg = create([0, 1, 2], [1, 2, 3], [1.0, 1.0, 1.0], _lib.ESP_MATRIX_FREE, fold=64)      # nothing is folded on this route
    assert st == _lib.BAD_ARG and "fold" in msg
    fi = np.arange(3)
    h = C.c_void_p()
    ci, cj, cw = i32([0]), i32([3]), f64([1.0])
    st = lib.machip_eig_create(0, 4, 3, p_i32(i32(fi)), p_i32(i32(fi + 1)), p_f64(f64(np.ones(3))), 1, p_i32(ci), p_i32(cj), p_f64(cw),
                               0, 0, _lib.ESP_MATRIX_FREE, C.byref(h))
    assert st == _lib.BAD_ARG and "MACHIP_ESP_MATRIX_FREE" in _lib.last_error()
