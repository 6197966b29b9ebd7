"""CPU checks of the shading-arithmetic switch (agpt_scene_set_shading_arith, include/agpt.h): the symbol is declared and
exported, the mode constants agree between the header and the binding, bad calls fail loudly with the function's name, and the
cross-compiled gfx950 code of the fast unit has given up the IEEE divide expansions and fp64 of its value arithmetic while the exact
unit keeps them."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

import ag_pathtracer_amd as ag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agpt_build", os.path.join(ROOT, "ag-pathtracer_amd", "build.py"))
b = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(b)
HEADER = open(os.path.join(ROOT, "include", "agpt.h")).read()
FAST_KERNELS = ["k_shade_fast<true, true>", "k_shade_fast<true, false>", "k_shade_fast<false, true>", "k_shade_fast<false, false>",
                "k_resolve_pending_fast", "k_kat_bsdf_eval_fast", "k_kat_bsdf_sample_fast", "k_kat_env_light_fast"]


def enum_value(name):
    m = re.search(r"\b%s\s*=\s*(-?\d+)" % name, HEADER)
    assert m, name
    return int(m.group(1))


def test_symbol_declared_and_exported():
    L = ag.lib()
    name = "agpt_scene_set_shading_arith"
    assert re.search(r"\b%s\s*\(" % name, HEADER)
    assert name in ag.EXPORTS
    assert hasattr(L, name)


def test_mode_constants_match_header():
    assert enum_value("AGPT_SHADING_EXACT") == ag.SHADING_EXACT == 0
    assert enum_value("AGPT_SHADING_FAST") == ag.SHADING_FAST == 1


def test_null_scene_is_invalid():
    L = ag.lib()
    assert L.agpt_scene_set_shading_arith(None, ag.SHADING_FAST) == enum_value("AGPT_ERR_INVALID")
    assert b"agpt_scene_set_shading_arith" in L.agpt_last_error()
    assert L.agpt_scene_set_shading_arith(None, 7) == enum_value("AGPT_ERR_INVALID")


def test_shade_variant_query_is_exported_and_refuses_null():
    """agpt_scene_shade_variant (host-only): declared, exported, and a NULL scene or output fails loudly with the function's name"""
    import ctypes
    L = ag.lib()
    name = "agpt_scene_shade_variant"
    assert re.search(r"\b%s\s*\(" % name, HEADER) and name in ag.EXPORTS and hasattr(L, name)
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    assert L.agpt_scene_shade_variant(None, out) == enum_value("AGPT_ERR_INVALID")
    assert b"agpt_scene_shade_variant" in L.agpt_last_error()
    assert list(out) == [7, 7, 7, 7]


def device_asm(src, tmp):
    """build.py's flags for `src`, device code only, as assembly."""
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    out = os.path.join(tmp, src + ".s")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + b.SOURCE_FLAGS.get(src, []) + \
        ["--cuda-device-only", "-S", "-o", out, os.path.join(b.CSRC, src)]
    return subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE), out


def functions(text):
    """{mangled name: instruction mnemonics} of every function (kernels and out-of-line device functions) in the assembly."""
    funcs = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.M | re.S):
        funcs[m.group(1)] = [ln.split()[0] for ln in m.group(2).split("\n")
                             if re.match(r"^\s+[a-z_][a-z_0-9]*", ln) and not ln.strip().startswith((".", ";"))]
    return funcs


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*", "", d).replace("void ", "") for n, d in zip(names, out)}


def is_div(mnemonic):
    return mnemonic.startswith(("v_div_scale_f32", "v_div_fixup_f32"))


def is_f64(mnemonic):
    return "_f64" in mnemonic


@pytest.fixture(scope="module")
def shade_asm():
    assert "agpt_shade_kernels_fast.hip" in b.SOURCES
    with tempfile.TemporaryDirectory() as tmp:
        jobs = {src: device_asm(src, tmp) for src in ("agpt_shade_kernels.hip", "agpt_shade_kernels_fast.hip")}
        texts = {}
        for src, (p, out) in jobs.items():
            _, err = p.communicate(timeout=600)
            assert p.returncode == 0, err.decode()[-2000:]
            texts[src] = open(out).read()
    return texts


def by_name(text):
    funcs = functions(text)
    pretty = demangle(list(funcs))
    return {pretty[n]: ops for n, ops in funcs.items()}


def test_fast_unit_relaxes_the_value_arithmetic(shade_asm):
    """The fast unit has every fast kernel.  What only computes values -- BSDF evaluation (k_kat_bsdf_eval_fast), the pending
    light samples (k_resolve_pending_fast) -- holds no IEEE divide expansion and no fp64; k_shade_fast keeps only the exact
    arithmetic of the sampled directions: at most half the divide expansions of k_shade."""
    fast = by_name(shade_asm["agpt_shade_kernels_fast.hip"])
    exact = by_name(shade_asm["agpt_shade_kernels.hip"])
    for k in FAST_KERNELS:
        assert k in fast, "%s missing from the fast unit (%s)" % (k, sorted(fast))
    for k in ("k_kat_bsdf_eval_fast", "k_resolve_pending_fast"):
        bad = sorted(set(op for op in fast[k] if is_div(op) or is_f64(op)))
        assert not bad, (k, bad)
    for inst in ("<true, true>", "<true, false>", "<false, true>", "<false, false>"):
        nf = sum(map(is_div, fast["k_shade_fast" + inst]))
        ne = sum(map(is_div, exact["k_shade" + inst]))
        assert 0 < ne and nf <= ne // 2, (inst, nf, ne)
        assert len([op for op in fast["k_shade_fast" + inst] if op.startswith("v_")]) < \
            len([op for op in exact["k_shade" + inst] if op.startswith("v_")])


def test_exact_kernels_keep_the_exact_arithmetic(shade_asm):
    """The switch must not leak into the default unit: its kernels still carry the IEEE divides and the fp64 trigonometry."""
    exact = by_name(shade_asm["agpt_shade_kernels.hip"])
    shade = [k for k in exact if k.startswith("k_shade<")]
    assert len(shade) == 4 and not any("_fast" in k for k in exact)
    for k in shade + ["k_resolve_pending"]:
        assert any(op.startswith("v_div_scale_f32") for op in exact[k]), k
        assert any(op.startswith("v_div_fixup_f32") for op in exact[k]), k
    for k in shade:
        assert any(is_f64(op) for op in exact[k]), k
