"""The C++ adapter's motion calls (include/agpt_host.hpp: Scene::SnapshotPositions, PathTracer::RenderFeaturesMotion,
AdaptiveAccumulator::TemporalAccumulate with Motion::Follow): examples/motion_scene.cpp compiled with g++ against libagpt_hip.so.  Its
moving mesh keeps history with the motion calls and none without."""
import re
import subprocess

import pytest

from helpers import build_cpp_example

W, H, FRAMES = 48, 40, 4


def test_cpp_motion_program_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "motion_scene")


@pytest.mark.gpu
def test_cpp_motion_history_follows_the_mesh(tmp_path):
    exe = build_cpp_example(tmp_path, "motion_scene")
    out = subprocess.check_output([exe, str(W), str(H), str(FRAMES)], timeout=300).decode()
    print(out)
    runs = {int(m): (int(n), int(h), float(c)) for m, n, h, c in
            re.findall(r"motion (\d) mesh_pixels (\d+) history (\d+) coverage ([0-9.]+)", out)}
    assert set(runs) == {0, 1}, out
    assert runs[0][0] == runs[1][0] >= 50                   # the same pixels show the mesh in both runs
    assert runs[1][1] > 0 and runs[1][2] > 0                # with the motion calls its history follows it
    assert runs[0][1] == 0 and runs[0][2] == 0.0            # without them the depth test rejects all of it
