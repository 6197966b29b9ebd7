"""The table of shading units (build.py: SHADE_UNITS) against the files it names and the level list of agpt_shade_kernels.h: a unit
that the table, its translation unit, the header and the build flags do not describe alike would compile and link, and the wrong
kernel would run."""
import importlib.util
import os
import re
import subprocess

import ag_pathtracer_amd as ag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agpt_build", os.path.join(ROOT, "ag-pathtracer_amd", "build.py"))
b = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(b)

LAUNCHERS = ["launch_shade", "launch_shade_fast", "launch_shade_textured", "launch_shade_textured_fast", "launch_shade_mapped",
             "launch_shade_mapped_fast", "launch_shade_sampled", "launch_shade_sampled_fast", "launch_shade_normal", "launch_shade_normal_fast"]
FLAGS_4_WAVES = ["-mllvm", "-disable-machine-licm", "-DAGPT_SHADE_WAVES=4"]
FLAGS_3_WAVES = ["-mllvm", "-disable-machine-licm", "-DAGPT_SHADE_WAVES=3"]


def unit_file(suffix):
    return "agpt_shade_kernels%s.hip" % suffix


def header_levels():
    """{level: suffix} of the header's level list"""
    text = open(os.path.join(b.CSRC, "agpt_shade_kernels.h")).read()
    line = re.search(r"^#define AGPT_SHADE_LEVEL_LIST\(X\)(.*)$", text, re.M).group(1)
    rows = re.findall(r"X\((\d+),\s*(\w*)\)", line)
    assert re.sub(r"X\(\d+,\s*\w*\)", "", line).strip() == "", line      # nothing but rows
    return {int(level): suffix for level, suffix in rows}


def test_ten_units_one_per_level_and_arithmetic():
    assert len(b.SHADE_UNITS) == 10
    assert sorted((level, fast) for _, level, fast, _ in b.SHADE_UNITS) == [(level, fast) for level in range(5) for fast in (0, 1)]


def test_each_unit_is_a_source_that_defines_its_row():
    for suffix, level, fast, _ in b.SHADE_UNITS:
        path = os.path.join(b.CSRC, unit_file(suffix))
        assert os.path.isfile(path), path
        assert b.SOURCES.count(unit_file(suffix)) == 1, suffix
        defines = dict(re.findall(r"^#define (AGPT_SHADE_LEVEL|AGPT_SHADE_FAST) (\d+)\s*$", open(path).read(), re.M))
        assert defines == {"AGPT_SHADE_LEVEL": str(level), "AGPT_SHADE_FAST": str(fast)}, (suffix, defines)
    assert [s for s in b.SOURCES if s.startswith("agpt_shade_kernels")] == [unit_file(u[0]) for u in b.SHADE_UNITS]


def test_unit_flags():
    for suffix, level, _, _ in b.SHADE_UNITS:
        assert b.SOURCE_FLAGS[unit_file(suffix)] == (FLAGS_3_WAVES if level == 4 else FLAGS_4_WAVES), suffix
    assert sorted(b.SOURCE_FLAGS) == sorted(unit_file(u[0]) for u in b.SHADE_UNITS)      # no other file has flags of its own


def test_header_names_a_launcher_for_each_unit():
    levels = header_levels()
    assert sorted(levels) == list(range(5))
    names = []
    for suffix, level, fast, _ in b.SHADE_UNITS:
        assert suffix == levels[level] + ("_fast" if fast else ""), (suffix, level, fast)
        names.append("launch_shade" + levels[level] + ("_fast" if fast else ""))
    assert names == LAUNCHERS


def test_library_defines_the_ten_launchers():
    """what AGPT_SHADE_KNAME made of launch_shade in each unit, read off the built library"""
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", ag.library_path()], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\bagpt::(launch_shade\w*)\(", out))) == sorted(LAUNCHERS)
