"""The C++ adapter's clamped temporal call (include/agpt_host.hpp: AdaptiveAccumulator::TemporalAccumulate with a clamp):
examples/clamped_scene.cpp compiled with g++ against libagpt_hip.so.  On the floor pixels the moved card's shadow left, the
accumulated history is closer to the new lighting with the clamp than without."""
import re
import subprocess

import pytest

from helpers import build_cpp_example

W, H = 64, 48


def test_cpp_clamped_program_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "clamped_scene")


@pytest.mark.gpu
def test_cpp_clamp_shortens_the_shadow_trail(tmp_path):
    exe = build_cpp_example(tmp_path, "clamped_scene")
    out = subprocess.check_output([exe, str(W), str(H)], timeout=300).decode()
    print(out)
    runs = {int(c): (int(n), float(e)) for c, n, e in re.findall(r"clamp (\d) uncovered (\d+) error ([0-9.]+)", out)}
    assert set(runs) == {0, 1}, out
    assert runs[0][0] == runs[1][0] >= 30                   # the same uncovered pixels in both runs
    assert runs[1][1] < runs[0][1]                          # and a smaller error with the clamp on
