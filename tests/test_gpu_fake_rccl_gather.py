"""agpt_gather_tiles with world > 1 -- the grouped send / recv into rank 0's staging buffer and the de-interleave behind it -- and
agpt_comm_init / agpt_comm_destroy with a communicator, on ONE GPU: every rank lives in one child process (tests/fake_rccl_driver.py) whose
nccl* functions are the stand-in transport tests/fake_rccl/fake_rccl.cpp.  agpt_comm.hip binds RCCL with dlopen("librccl.so.1"), and the
child has loaded the stand-in, whose SONAME that is, before the library: no production code knows about the test.  The stand-in only
queues inside a group, runs the queue at the group's end (an event on the sender's stream, a wait and a device-to-device copy on the
receiver's), never synchronises the host, logs every call and can be told to fail one.  What is checked is this repository's side: the
per-rank counts, the staging slot size and offsets, the ranks that own nothing, that a started group is always ended, the stream, the
order against k_deinterleave, the error reports.  RCCL's own transfer is not.

The expected film is the random film the compact buffers were cut from in numpy (the inverse row-block mapping), never another call of
the code under test; every comparison is of bytes.  The driver runs once per module; with this pytest process two processes hold the GPU.
Measured on an MI355X: the driver takes 1.1 s of wall time (DRIVER_SECONDS), the interpreter's start and the cold start of
the HIP runtime included; the limit is ten times that and not under 60 s, so 60 s."""
import json
import os
import subprocess
import sys
import time

import pytest

import fake_rccl_driver as drv
import hip_runtime
from helpers import ROOT, build_cpp_example, build_fake_rccl

pytestmark = pytest.mark.gpu

DRIVER_SECONDS = 1.1          # measured wall time of the driver, see above
DRIVER_LIMIT = max(60.0, 10 * DRIVER_SECONDS)
AGPT_ERR_INVALID, AGPT_ERR_DEVICE = -1, -2      # include/agpt.h
SYSTEM_ERROR = drv.ERROR_STRINGS[drv.NCCL_SYSTEM_ERROR]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """{"stand_in": path, "failure": why nothing can be read (None: the JSON is there), "json": the driver's results}"""
    tmp = tmp_path_factory.mktemp("fake_rccl")
    rec = {"stand_in": build_fake_rccl(tmp), "failure": None, "json": None}
    out = tmp / "driver.json"
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fake_rccl_driver.py"), rec["stand_in"], str(out)], timeout=DRIVER_LIMIT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        rec["failure"] = "the driver did not end within %.0f s: %s" % (DRIVER_LIMIT, e.stdout)
        return rec
    print("driver: %.1f s of wall time, exit status %d\n%s" % (time.perf_counter() - t0, p.returncode, p.stdout))
    if p.returncode < 0:
        rec["failure"] = "the driver ended on signal %d: %s" % (-p.returncode, p.stdout)
    elif not out.exists():
        rec["failure"] = "the driver left no results (exit status %d): %s" % (p.returncode, p.stdout)
    else:
        rec["json"] = json.loads(out.read_text())
    return rec


def results(run):
    assert run["failure"] is None, run["failure"]
    return run["json"]


def case(run, name):
    j = results(run)
    assert name in j["cases"], "the driver did not reach %s: %s" % (name, j["exception"])
    return j["cases"][name]


def rows_of(H, block, world, rank):
    """rows of the film's row blocks k (of `block` rows, the last one short) with k % world == rank"""
    return sum(min(block, H - k * block) for k in range(rank, -(-H // block), world))


def calls_of(lines):
    return [ln for ln in lines if ln["fn"] != "ERROR"]


def check_gather(rec, streams=None):
    """one clean gather's record: the film, and from the log every rank's calls"""
    W, H, block, world = rec["W"], rec["H"], rec["block"], rec["world"]
    assert rec["film"] == {"exact": True, "pixels_differing": 0, "pixels_still_ff": 0}, rec["film"]
    rows = [rows_of(H, block, world, r) for r in range(world)]
    assert sum(rows) == H
    stream = lambda r: streams[r] if streams else 0
    sent = 0
    for r in range(world):
        lines = rec["calls"][str(r)]
        assert all(ln["fn"] != "ERROR" and ln["rc"] == 0 for ln in lines), (r, lines)
        assert rec["status"][str(r)] == [0, ""] and rec["depth"][str(r)] == 0, r
        assert (lines[0]["fn"], lines[0]["depth"]) == ("GroupStart", 1) and (lines[-1]["fn"], lines[-1]["depth"]) == ("GroupEnd", 0), (r, lines)
        inner = lines[1:-1]
        if r:
            # a peer: one send of its own rows to rank 0 -- never its whole buffer, whose rows past the share hold the sentinel -- or none
            want = [("Send", r, 0, rows[r] * W * 4, drv.NCCL_FLOAT, stream(r))] if rows[r] else []
        else:
            want = [("Recv", 0, p, rows[p] * W * 4, drv.NCCL_FLOAT, stream(0)) for p in range(1, world) if rows[p]]
        assert [(ln["fn"], ln["rank"], ln["peer"], ln["count"], ln["dtype"], ln["stream"]) for ln in inner] == want, (r, inner, want)
        if r:
            sent += sum(ln["count"] for ln in inner)
    assert sent + rows[0] * W * 4 == W * H * 4


@pytest.mark.parametrize("shape", drv.GATHER_CASES, ids=lambda s: drv.case_name(*s))
def test_gather(run, shape):
    """the table: (5, 37, 8, 3) shares of 16, 13 and 8 rows, rank 1 ends in a short block and its staging slot is larger than what it
    sends; (96, 77, 8, 3) test_gpu_gather_tiles_c_abi's shape; (3, 8, 8, 4) one block, ranks 1..3 own nothing; (7, 1, 8, 2) a single row;
    (64, 64, 8, 8) an even split; (33, 50, 4, 5) a block height other than 8; (1, 1080, 8, 8) the production split"""
    W, H, block, world = shape
    rec = case(run, drv.case_name(*shape))
    check_gather(rec)
    opened = rec["opened"]
    assert [(ln["fn"], ln["rc"]) for ln in opened] == [("GetUniqueId", 0)] + [("CommInitRank", 0)] * world, opened
    assert [(ln["rank"], ln["count"]) for ln in opened[1:]] == [(r, world) for r in range(world)]
    assert [(ln["fn"], ln["rank"], ln["rc"]) for ln in rec["closed"]] == [("CommDestroy", r, 0) for r in range(world)], rec["closed"]
    assert rec["live_comms_after"] == 0


def test_the_shares_the_table_names():
    assert [rows_of(37, 8, 3, r) for r in range(3)] == [16, 13, 8]
    assert [rows_of(8, 8, 4, r) for r in range(4)] == [8, 0, 0, 0]
    assert [rows_of(1080, 8, 8, r) for r in range(8)] == [17 * 8] * 7 + [16 * 8]
    assert [rows_of(50, 4, 5, r) for r in range(5)] == [12, 12, 10, 8, 8]


def test_ranks_without_rows_neither_send_nor_are_received_from(run):
    rec = case(run, drv.case_name(3, 8, 8, 4))
    for r in range(4):
        assert [ln["fn"] for ln in rec["calls"][str(r)]] == ["GroupStart", "GroupEnd"], r     # (the group is still started and ended)


def test_staging_grows_and_the_slot_size_changes_back(run):
    recs = case(run, "regrow")
    assert [(r["W"], r["H"]) for r in recs] == [(5, 37), (96, 77), (5, 37)]
    for rec in recs:
        check_gather(rec)


def test_transfers_are_on_each_ranks_own_stream(run):
    rec = case(run, "streams")
    streams = rec["streams"]
    assert len(set(streams)) == 3 and all(streams)
    check_gather(rec, streams)


def test_rendered_shares_gather_to_the_whole_film_render(run):
    rec = case(run, "render")
    assert rec["lit_pixels"] > 96 * 77 // 2
    assert rec["exact"] and rec["pixels_differing"] == 0 and rec["depth"] == 0, rec


def test_only_the_streams_order_the_gather_behind_its_inputs(run):
    """test_gpu_streams.py's pattern at world 3: each rank's compact buffer gets its values from a copy on the rank's stream behind a delay
    that the host never waits for, and every rank's stream is still busy when its agpt_gather_tiles is called"""
    rec = case(run, "streams_delay")
    assert rec["busy"] == {str(r): hip_runtime.hipErrorNotReady for r in range(3)}, (rec["busy"], rec["delay_ms"])
    check_gather(rec, rec["streams"])


# what the failing rank's own call logs, and how many sends of the ranks before it no receive took
FAULT_CALLS = {"Recv@0": (["GroupStart", "Recv", "GroupEnd"], 2), "Send@1": (["GroupStart", "Send", "GroupEnd"], 0),
               "GroupStart@0": (["GroupStart"], 2), "GroupStart@2": (["GroupStart"], 1),
               "GroupEnd@0": (["GroupStart", "Recv", "Recv", "GroupEnd"], 2), "GroupEnd@1": (["GroupStart", "Send", "GroupEnd"], 0)}


@pytest.mark.parametrize("fault", ["%s@%d" % f for f in drv.FAULTS])
def test_a_failed_transport_call_is_reported_and_leaves_nothing_open(run, fault):
    rec = case(run, "faults")[fault]
    fn, rank = fault.split("@")
    fns, left = FAULT_CALLS[fault]
    status, message = rec["status"][rank]
    assert status == AGPT_ERR_DEVICE and "agpt_gather_tiles" in message and SYSTEM_ERROR in message, (status, message)
    lines = rec["calls"][rank]
    assert [ln["fn"] for ln in lines] == fns, lines
    failed = [ln for ln in lines if ln["rc"]]
    assert [(ln["fn"], ln["rc"]) for ln in failed] == [(fn, drv.NCCL_SYSTEM_ERROR)], lines
    if fn in ("Send", "Recv"):
        assert lines.index(failed[0]) < len(lines) - 1 and lines[-1]["fn"] == "GroupEnd"     # the group was ended behind the failure
    assert lines[-1]["depth"] == 0 and rec["depth"][rank] == 0
    assert rec["sends_left_posted"] == left
    check_gather(rec["clean"])


def test_an_error_of_the_groups_end_is_the_one_reported(run):
    """rank 0 alone: its receives are queued without complaint and only the end of the group finds that nothing was sent"""
    rec = case(run, "no_sends")
    status, message = rec["status"]["0"]
    assert status == AGPT_ERR_DEVICE and drv.ERROR_STRINGS[drv.NCCL_INTERNAL_ERROR] in message, (status, message)
    lines = rec["calls"]["0"]
    assert [(ln["fn"], ln["rc"]) for ln in calls_of(lines)] == [("GroupStart", 0), ("Recv", 0), ("Recv", 0), ("GroupEnd", drv.NCCL_INTERNAL_ERROR)]
    assert sum(ln["fn"] == "ERROR" for ln in lines) == 1 and rec["depth"]["0"] == 0
    check_gather(rec["clean"])


def test_arguments(run):
    a = case(run, "arguments")
    assert a["rank0_null_full"]["status"][0] == AGPT_ERR_INVALID and a["rank0_null_full"]["calls"] == []
    assert [s[0] for s in a["peer_null_full"]["status"]] == [0, 0]
    assert [ln["fn"] for ln in a["peer_null_full"]["calls"]] == ["GroupStart", "Send", "GroupEnd"] * 2
    assert a["then_rank0"]["status"][0] == 0 and a["then_rank0"]["film"]["exact"] and a["then_rank0"]["film"]["pixels_still_ff"] == 0
    assert a["init_null_id"] == {"status": AGPT_ERR_INVALID, "handle": None, "calls": []}
    assert [(ln["fn"], ln["rank"], ln["rc"]) for ln in a["close"]["calls"]] == [("CommDestroy", r, 0) for r in range(3)], a["close"]
    assert a["close"]["live_comms_after"] == 0


def test_the_driver_ran_to_its_end_on_the_stand_in(run):
    j = results(run)
    assert j["exception"] is None, j["exception"]
    assert [ln["fn"] for ln in j["bound"]["lines"]] == ["GetUniqueId"] and bytes.fromhex(j["bound"]["id"]).startswith(drv.ID_TAG)
    assert j["torch_imported"] is False and j["depth_at_end"] == 0
    assert j["seconds"] < DRIVER_LIMIT


CPP_PROGRAM = r"""
// (5, 37, 8, 3) through agpt::Comm::UniqueId, agpt::Comm and GatherTiles, one agpt::Context per rank, over the stand-in transport
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "agpt_host.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    void* lib = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
    if (!lib) {
        std::fprintf(stderr, "dlopen: %s\n", dlerror());
        return 2;
    }
    const int W = 5, H = 37, world = 3, max_rows = 16;
    const std::vector<unsigned char> id = agpt::Comm::UniqueId();
    if (std::memcmp(id.data(), "FAKE-RCCL-ID", 12) != 0) {
        std::fprintf(stderr, "the real librccl was bound\n");
        return 3;
    }
    std::vector<std::unique_ptr<agpt::Context>> ctx;
    std::vector<std::unique_ptr<agpt::Accumulator>> local;
    std::vector<std::unique_ptr<agpt::Comm>> comm;
    std::vector<agpt::RankShare> share;
    for (int r = 0; r < world; r++) {
        ctx.emplace_back(new agpt::Context(0));
        agpt::RankShare s;
        s.world = world;
        s.rank = r;
        share.push_back(s);
        local.emplace_back(new agpt::Accumulator(*ctx[r], W, max_rows));
        std::vector<unsigned char> bytes((size_t)W * max_rows * 16);
        FILE* f = std::fopen((std::string(argv[2]) + "/rank" + std::to_string(r) + ".bin").c_str(), "rb");
        if (!f || std::fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) return 2;
        std::fclose(f);
        agpt::check(agpt_device_upload(ctx[r]->handle(), local[r]->device_pixels(), bytes.data(), bytes.size()), "agpt_device_upload");
        comm.emplace_back(new agpt::Comm(*ctx[r], id, world, r));
    }
    unsigned long long hash = 14695981039346656037ull;
    {
        agpt::Accumulator full(*ctx[0], W, H);
        for (int r : {1, 2, 0}) comm[r]->GatherTiles(*local[r], H, share[r], r == 0 ? &full : nullptr);
        const std::vector<float> film = full.Download();
        const unsigned char* p = reinterpret_cast<const unsigned char*>(film.data());
        for (size_t i = 0; i < film.size() * 4; i++) hash = (hash ^ p[i]) * 1099511628211ull;
    }
    comm.clear();
    int (*depth)() = reinterpret_cast<int (*)()>(dlsym(lib, "fake_rccl_group_depth"));
    int (*live)() = reinterpret_cast<int (*)()>(dlsym(lib, "fake_rccl_live_comms"));
    std::printf("%016llx depth %d live %d\n", hash, depth(), live());
    return 0;
}
"""


def fnv1a(data):
    h = 14695981039346656037
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_adapter(run, tmp_path):
    """include/agpt_host.hpp's Comm over the stand-in, in a process of its own that dlopens the stand-in first"""
    results(run)                                  # (nothing more is started on the GPU if the driver timed out or died)
    from ag_pathtracer_amd import tiles
    W, H, block, world = 5, 37, 8, 3
    film = drv.make_film(W, H, 600)
    for r in range(world):
        (tmp_path / ("rank%d.bin" % r)).write_bytes(drv.compact_of(film, tiles, H, W, block, world, r).tobytes())
    src = tmp_path / "fake_rccl_gather.cpp"
    src.write_text(CPP_PROGRAM)
    exe = build_cpp_example(tmp_path, str(src))
    p = subprocess.run([exe, run["stand_in"], str(tmp_path)], timeout=DRIVER_LIMIT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.split() == ["%016x" % fnv1a(film.tobytes()), "depth", "0", "live", "0"], p.stdout
