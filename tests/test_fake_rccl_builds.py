"""The stand-in transport of test_gpu_fake_rccl_gather.py (tests/fake_rccl/fake_rccl.cpp), without a GPU: it compiles against the real
<rccl/rccl.h>, exports exactly the nccl* functions that agpt_comm.hip binds under the SONAME that file asks dlopen for, and keeps its own
rules where no HIP call is involved.  A function added to AGPT_RCCL_FUNCTIONS fails here, by its name, and not as "librccl.so could not be
loaded" on a GPU.  The stand-in is never loaded into this process (its SONAME would answer a later dlopen("librccl.so.1") here): its
behaviour is read from a child process."""
import json
import os
import re
import subprocess
import sys

import pytest

import fake_rccl_driver as drv
from helpers import ROOT, build_fake_rccl


@pytest.fixture(scope="module")
def stand_in(tmp_path_factory):
    return build_fake_rccl(tmp_path_factory.mktemp("fake_rccl"))


def bound_functions():
    src = open(os.path.join(ROOT, "ag-pathtracer_amd", "csrc", "agpt_comm.hip")).read()
    m = re.search(r"#define AGPT_RCCL_FUNCTIONS\(X\)(.*)", src)
    names = re.findall(r"X\((\w+)\)", m.group(1))
    assert len(names) >= 8 and len(set(names)) == len(names), names
    return names


def test_exports_exactly_the_bound_functions(stand_in):
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", stand_in]).decode()
    exported = {ln.split()[-1] for ln in dyn.splitlines() if ln.strip()}
    nccl = {s for s in exported if "nccl" in s.lower()}
    for name in bound_functions():
        assert "nccl" + name in nccl, "the stand-in lacks nccl%s, which agpt_comm.hip binds" % name
    assert nccl == {"nccl" + n for n in bound_functions()}, sorted(nccl)
    for s in ("fake_rccl_log_count", "fake_rccl_log_line", "fake_rccl_fail_nth", "fake_rccl_reset", "fake_rccl_group_depth"):
        assert s in exported, s


def test_soname_is_what_agpt_comm_asks_for(stand_in):
    dynamic = subprocess.check_output(["readelf", "-d", stand_in]).decode()
    assert re.findall(r"\(SONAME\).*\[(.*)\]", dynamic) == ["librccl.so.1"]
    src = open(os.path.join(ROOT, "ag-pathtracer_amd", "csrc", "agpt_comm.hip")).read()
    first = re.search(r'for \(const char\* name : \{"([^"]+)"', src)
    assert first and first.group(1) == "librccl.so.1"      # the name the library tries first


def test_rules_that_need_no_gpu(stand_in, tmp_path):
    out = tmp_path / "selfcheck.json"
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fake_rccl_driver.py"), stand_in, str(out), "selfcheck"], check=True, timeout=120)
    got = json.loads(out.read_text())
    assert got["send_outside_group"] == drv.NCCL_INVALID_USAGE
    assert got["end_without_start"] == drv.NCCL_INVALID_USAGE
    assert got["pair"] == [0, 1, 0, 2, 0, 1, 0, 0]
    # armed for the second GroupStart: the first passes, the second fails and opens nothing, the third passes again
    assert got["fault"] == [0, 0, drv.NCCL_SYSTEM_ERROR, 0, 0, 0, 0]
    assert len(set(got["strings"])) == 8
    for code, text in drv.ERROR_STRINGS.items():
        assert got["strings"][code] == text
    a, b = (bytes.fromhex(x) for x in got["ids"])
    assert len(a) == len(b) == 128 and a != b and a.startswith(drv.ID_TAG) and b.startswith(drv.ID_TAG)
    log = got["log"]
    assert [ln["fn"] for ln in log] == ["Send", "GroupEnd"] + ["GroupStart", "GroupStart", "GroupEnd", "GroupEnd"] + \
        ["GroupStart", "GroupEnd", "GroupStart", "GroupStart", "GroupEnd"] + ["GetUniqueId", "GetUniqueId"]
    assert log[0]["rc"] == drv.NCCL_INVALID_USAGE and log[0]["count"] == 4 and log[0]["dtype"] == drv.NCCL_FLOAT and log[0]["depth"] == 0
    assert [ln["depth"] for ln in log[2:6]] == [1, 2, 1, 0]
    assert got["reset"] == [0, 0]
