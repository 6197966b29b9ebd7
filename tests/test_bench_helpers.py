"""bench.py's bookkeeping that does not need a GPU: which committed PMC profile a run may use for its per-ray constants."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_pmc_profile_is_keyed_by_kernel_build_and_workload(tmp_path, monkeypatch):
    prof = tmp_path / "profiles"
    prof.mkdir()
    mk = lambda name, build, wl, extra=None: (prof / name).write_text(json.dumps(dict(kernel_build=build, workload=wl, trace={"valu_insts_per_traversed_ray": 1.0},
                                                                                     **(extra or {}))))
    mk("pmc_a.json", "BUILD", "c3:1920x1080:64spp:world1:scale1")
    mk("pmc_b.json", "OTHER", "c3:1920x1080:64spp:world1:scale1")
    mk("pmc_c.json", "BUILD", "c5:1920x1080:64spp:world1:scale1")
    (prof / "pmc_l1.json").write_text(json.dumps(dict(kernel_build="BUILD", workload="c3:1920x1080:64spp:world1:scale1")))   # no "trace": not a roofline profile
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_build_id", lambda: "BUILD")
    p = bench.load_pmc_profile("c3:1920x1080:64spp:world1:scale1")
    assert p and p["file"].endswith("pmc_a.json") and p["stand_in"] is False
    # a rank's share of the same film: the whole film's per-ray constants stand in, flagged
    p = bench.load_pmc_profile("c3:1920x1080:64spp:world8:scale1")
    assert p and p["file"].endswith("pmc_a.json") and p["stand_in"] is True
    # an own profile of the split wins over the stand-in
    mk("pmc_d.json", "BUILD", "c3:1920x1080:64spp:world8:scale1")
    p = bench.load_pmc_profile("c3:1920x1080:64spp:world8:scale1")
    assert p and p["file"].endswith("pmc_d.json") and p["stand_in"] is False
    # other film, other sample count, other build: nothing
    assert bench.load_pmc_profile("c3:1920x1080:8spp:world2:scale1") is None
    assert bench.load_pmc_profile("c3:3840x2160:64spp:world1:scale1") is None
    monkeypatch.setattr(bench, "kernel_build_id", lambda: "NEWER")
    assert bench.load_pmc_profile("c3:1920x1080:64spp:world1:scale1") is None


def test_kernel_build_id_covers_every_kernel_source():
    """The id profiles are keyed by is a hash over csrc/ and build.py: a new translation unit or header is part of it."""
    import inspect
    src = inspect.getsource(bench.kernel_build_id)
    assert "csrc" in src and "build.py" in src
    a = bench.kernel_build_id()
    assert len(a) == 16 and a == bench.kernel_build_id()


def test_dump_outputs_writes_the_film_and_the_ray_counts(tmp_path):
    import numpy as np
    acc = np.arange(6 * 5 * 4, dtype=np.float32).reshape(6, 5, 4)
    bench.dump_outputs(str(tmp_path / "out"), acc, [7, 5, 3])
    a = np.load(tmp_path / "out" / "accum.npy")
    assert a.dtype == np.float32 and np.array_equal(a, acc)
    c = np.load(tmp_path / "out" / "ray_counts.npy")
    assert c.dtype == np.float64 and c.tolist() == [7.0, 5.0, 3.0]


def test_dump_outputs_samples_a_film_above_64_mb_the_same_way_every_time(tmp_path):
    import numpy as np
    H, W = 2160, 3840
    acc = np.repeat(np.arange(H * W, dtype=np.float32).reshape(H, W, 1), 4, axis=2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), acc, [1, 2, 3])
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["accum_sample.npy", "accum_sample_pixels.npy", "ray_counts.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= 64 << 20
    s, i = np.load(tmp_path / "a" / "accum_sample.npy"), np.load(tmp_path / "a" / "accum_sample_pixels.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64 and len(s) == len(i) == bench.DUMP_SAMPLE_PIXELS
    assert np.array_equal(s[:, 0], i.astype(np.float32)) and np.all(np.diff(i) > 0)
    assert np.array_equal(i, np.load(tmp_path / "b" / "accum_sample_pixels.npy"))
