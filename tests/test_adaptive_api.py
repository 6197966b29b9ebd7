"""CPU checks of adaptive sampling (agpt_render_adaptive): the C structs against their ctypes mirrors, the numpy model of the
contract on hand-made sample sets, argument checks that need no GPU, and the new unit's cross-compiled resources."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_model as am
import ag_pathtracer_amd as ag
from helpers import assert_exported, struct_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agpt_build", os.path.join(ROOT, "ag-pathtracer_amd", "build.py"))
b = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(b)


def test_symbols_declared_and_exported():
    assert_exported(("agpt_render_adaptive", "agpt_resolve_counts"))
    assert "agpt_adaptive.hip" in b.SOURCES


def test_struct_layout_matches_ctypes(tmp_path):
    struct_layout(tmp_path, {"agpt_adaptive_params": ag.AdaptiveParams, "agpt_adaptive_stats": ag.AdaptiveStats})


def test_null_arguments_are_invalid_without_a_gpu():
    L = ag.lib()
    rp, ap = ag.RenderParams(), ag.AdaptiveParams(4, 32, 4, 0.1, 0.0)
    invalid = -1
    assert L.agpt_render_adaptive(None, C.byref(rp), C.byref(ap), None, None, None, None) == invalid
    assert b"agpt_render_adaptive" in L.agpt_last_error()
    assert L.agpt_resolve_counts(None, None, 16, None) == invalid


# ---- the model -----------------------------------------------------------------------------------------------------
def test_model_constant_samples_stop_at_min_spp():
    rng = np.random.RandomState(1)
    vals = rng.uniform(0.1, 2.0, (6, 5, 3)).astype(np.float32)
    samples = np.broadcast_to(vals, (32, 6, 5, 3))
    r = am.run(samples, 8, 32, 4, 0.01)
    assert (r["counts"] == 8).all()
    # sums in sample order, float32
    ref = np.zeros((6, 5, 3), np.float32)
    for s in range(8):
        ref = ref + vals
    assert r["accum"].tobytes() == ref.tobytes()
    assert r["rounds"] == 2


def test_model_rel_error_off_goes_to_max_spp():
    rng = np.random.RandomState(2)
    samples = rng.uniform(0, 1, (24, 4, 4, 3)).astype(np.float32)
    for rel in (0.0, -1.0):
        r = am.run(samples, 4, 24, 4, rel)
        assert (r["counts"] == 24).all()
        ref = np.zeros((4, 4, 3), np.float32)
        m = np.zeros((4, 4), np.float32)
        for s in range(24):
            ref = ref + samples[s]
            y = am.luminance(samples[s])
            m = m + y * y
        assert r["accum"].tobytes() == ref.tobytes()
        assert r["moment2"].tobytes() == m.tobytes()


def test_model_high_variance_pixel_runs_to_the_cap():
    rng = np.random.RandomState(3)
    samples = np.full((64, 3, 3, 3), 0.5, np.float32)
    # pixel (1, 1): a rare bright sample every 7th -- the error estimate never falls below 1 %
    samples[::7, 1, 1] = 50.0
    # pixel (0, 2): mild noise that converges half-way
    samples[:, 0, 2] = rng.uniform(0.45, 0.55, (64, 3))
    r = am.run(samples, 4, 64, 4, 0.01)
    c = r["counts"]
    assert c[1, 1] == 64
    assert c[0, 0] == 4
    assert 4 < c[0, 2] < 64
    assert c[0, 2] % 4 == 0


def test_model_nan_samples_are_rejected_and_continuation_matches_one_call():
    rng = np.random.RandomState(4)
    samples = rng.exponential(1.0, (32, 5, 7, 3)).astype(np.float32)
    samples[3, 2, 2, 1] = np.nan
    samples[9, 4, 6, 0] = np.inf
    one = am.run(samples, 4, 32, 4, 0.2, 0.01)
    assert one["outliers"] == 2
    first = am.run(samples, 4, 16, 4, 0.2, 0.01)
    second = am.run(samples, 4, 32, 4, 0.2, 0.01, counts=first["counts"], accum=first["accum"], moment2=first["moment2"])
    assert np.array_equal(one["counts"], second["counts"])
    assert one["accum"].tobytes() == second["accum"].tobytes()
    assert one["moment2"].tobytes() == second["moment2"].tobytes()
    assert len(np.unique(one["counts"])) >= 3


def test_model_stop_test_formula():
    # two samples of luminance 1 and 3 (grey): mu = 2, unbiased var = 2, sqrt(var / n) = 1
    S = np.array([[4.0, 4.0, 4.0]], np.float32)
    M = np.array([10.0], np.float32)
    lhs, rhs = am.test_value(S, M, np.array([2]), 0.5, 0.0)
    assert abs(float(lhs[0]) - 1.0) < 1e-6 and abs(float(rhs[0]) - 1.0) < 1e-6
    act, _ = am.decide(S, M, np.array([2]), 2, 8, 0.49, 0.0)
    assert act[0]
    act, _ = am.decide(S, M, np.array([2]), 2, 8, 0.51, 0.0)
    assert not act[0]
    # the floor: a dark pixel stops against abs_floor
    act, _ = am.decide(S * 0, M * 0, np.array([2]), 2, 8, 0.1, 0.0)
    assert not act[0]


# ---- the unit cross-compiles for gfx950 without scratch ----------------------------------------------------------------
def test_adaptive_unit_compiles_without_scratch():
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "agpt_adaptive.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + b.SOURCE_FLAGS.get("agpt_adaptive.hip", []) + \
            ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out, os.path.join(b.CSRC, "agpt_adaptive.hip")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"remark: Function Name: (\S+)", p.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    assert len(names) == len(scratch) and len(names) >= 5
    for k in ("k_adaptive_select", "k_adaptive_compact", "k_generate_list", "k_accumulate_list", "k_resolve_counts"):
        assert any(k in n for n in names), (k, names)
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
