"""The trace kernels' translation unit (agpt_trace_kernels.hip) against the cross-compiled gfx950 code: it holds exactly the 40
k_trace_fast, 8 k_trace and 3 k_candidates instantiations that launch_trace picks among, built with the library's common flags, and
agpt_api.hip holds none of them -- only the five small kernels it launches itself.  Two device-only compiles, no GPU."""
import importlib.util
import itertools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agpt_build", os.path.join(ROOT, "ag-pathtracer_amd", "build.py"))
b = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(b)

TRACE_UNIT = "agpt_trace_kernels.hip"
API_UNIT = "agpt_api.hip"
TRACE_FAMILIES = ("k_trace_fast", "k_trace", "k_candidates")
API_KERNELS = ["k_prepare_rays", "k_export_hits", "k_generate", "k_generate_li", "k_resolve"]


def device_asm(src, tmp):
    """build.py's flags for `src`, device code only, as assembly (the technique of test_shading_arith_api.py)."""
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    out = os.path.join(tmp, src + ".s")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + b.SOURCE_FLAGS.get(src, []) + \
        ["--cuda-device-only", "-S", "-o", out, os.path.join(b.CSRC, src)]
    return subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE), out


@pytest.fixture(scope="module")
def kernels():
    """{unit: [(family, template arguments as a tuple of strings)]} of the .amdhsa_kernel entries of the two units"""
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        jobs = {src: device_asm(src, tmp) for src in (TRACE_UNIT, API_UNIT)}
        for src, (proc, out) in jobs.items():
            err = proc.communicate()[1]
            assert proc.returncode == 0, err.decode()
            mangled = re.findall(r"^\s*\.amdhsa_kernel (\S+)", open(out).read(), re.M)
            pretty = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
            result[src] = []
            for name in pretty[:len(mangled)]:
                m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?(\w+)(?:<([^>]*)>)?\(", name)
                assert m, name
                result[src].append((m.group(1), tuple(a.strip() for a in m.group(2).split(",")) if m.group(2) else ()))
    return result


def fast_stack():
    text = open(os.path.join(b.CSRC, "agpt_internal.h")).read()
    return re.search(r"^#define AGPT_FAST_STACK (\d+)\s*$", text, re.M).group(1)


def test_trace_unit_is_a_source_without_flags_of_its_own():
    assert b.SOURCES.count(TRACE_UNIT) == 1
    assert os.path.isfile(os.path.join(b.CSRC, TRACE_UNIT))
    assert TRACE_UNIT not in b.SOURCE_FLAGS


def test_trace_unit_holds_exactly_the_51_trace_kernels(kernels):
    families = [family for family, _ in kernels[TRACE_UNIT]]
    assert sorted(set(families)) == sorted(TRACE_FAMILIES), sorted(set(families))
    assert {f: families.count(f) for f in TRACE_FAMILIES} == {"k_trace_fast": 40, "k_trace": 8, "k_candidates": 3}
    assert len(set(kernels[TRACE_UNIT])) == 51      # no instantiation twice


def test_the_forty_k_trace_fast_instantiations(kernels):
    """<MODE, DEPTH, LIST, COUNT, SPILL, PEEK, COH>: 3 modes x short / long list x the six <COUNT, SPILL, PEEK> with COUNT and PEEK
    never both set, plus the four coherent ones (mode 0, short list, no COUNT), every one at depth AGPT_FAST_STACK"""
    depth = fast_stack()
    tf = {"0": "false", "1": "true"}
    csp = [(c, s, p) for c, s, p in itertools.product("01", repeat=3) if not (c == "1" and p == "1")]
    assert len(csp) == 6
    want = [(mode, depth, tf[lst], tf[c], tf[s], tf[p], "false") for mode in "012" for lst in "01" for c, s, p in csp]
    want += [("0", depth, "false", "false", tf[s], tf[p], "true") for s in "01" for p in "01"]
    assert len(want) == 40
    got = [args for family, args in kernels[TRACE_UNIT] if family == "k_trace_fast"]
    assert sorted(got) == sorted(want)


def test_api_unit_defines_no_trace_kernel_and_keeps_its_own_five(kernels):
    names = [family for family, _ in kernels[API_UNIT]]
    assert not [n for n in names if n in TRACE_FAMILIES], names
    for k in API_KERNELS:
        assert names.count(k) == 1, (k, names)
