"""The child process of test_gpu_fake_rccl_gather.py (and, with a third argument "selfcheck", of test_fake_rccl_builds.py): every rank of a
multi-rank agpt_gather_tiles in ONE process on ONE GPU, over the stand-in transport tests/fake_rccl/fake_rccl.cpp.

    python tests/fake_rccl_driver.py STAND_IN.so OUT.json [selfcheck]

The stand-in (SONAME librccl.so.1) is loaded first, by its path and with RTLD_GLOBAL; only then is ag_pathtracer_amd imported, whose
library binds nccl* with dlopen("librccl.so.1") and so gets the object that is already there.  torch is never imported.  The first call
is comm_unique_id(): unless the stand-in logged it and its tag is in the bytes, the process ends at once with "the real librccl was
bound".  One ag.Context per rank, as a real host has; for each gather the peers are called first and rank 0 last (the stand-in's
receive takes what a send has posted).  The process stops at the first exception and writes what it has.  Not collected by pytest."""
import ctypes as C
import json
import os
import sys
import time
import traceback

import numpy as np

ID_TAG = b"FAKE-RCCL-ID"
NCCL_FLOAT = 7
NCCL_SYSTEM_ERROR, NCCL_INTERNAL_ERROR, NCCL_INVALID_USAGE = 2, 3, 5
ERROR_STRINGS = {NCCL_SYSTEM_ERROR: "fake rccl: unhandled system error", NCCL_INTERNAL_ERROR: "fake rccl: internal error"}
SENTINEL = 0xDEADBEEF       # the bits of every float in a compact row past the rank's share
# (W, H, block, world): what each shape is there for is said at test_gpu_fake_rccl_gather.py's test_gather
GATHER_CASES = [(5, 37, 8, 3), (96, 77, 8, 3), (3, 8, 8, 4), (7, 1, 8, 2), (64, 64, 8, 8), (33, 50, 4, 5), (1, 1080, 8, 8)]
# (function that fails, rank whose call it fails in): the gather stops behind that rank, then a clean one runs
FAULTS = [("Recv", 0), ("Send", 1), ("GroupStart", 0), ("GroupStart", 2), ("GroupEnd", 0), ("GroupEnd", 1)]


def case_name(W, H, block, world):
    return "%dx%d_b%d_w%d" % (W, H, block, world)


def parse_line(line):
    """one call line of the stand-in's log -> dict (an ERROR line -> {"fn": "ERROR", "text": ...})"""
    if line.startswith("ERROR "):
        return {"fn": "ERROR", "text": line[6:]}
    parts = line.split()
    d = {"fn": parts[0]}
    for kv in parts[1:]:
        k, v = kv.split("=")
        d[k] = (0 if v == "(nil)" else int(v, 16)) if k == "stream" else int(v)
    return d


class StandIn:
    def __init__(self, path):
        L = self.L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        L.fake_rccl_log_line.argtypes = [C.c_int]
        L.fake_rccl_log_line.restype = C.c_char_p
        L.fake_rccl_fail_nth.argtypes = [C.c_char_p, C.c_int]
        L.fake_rccl_fail_nth.restype = None
        L.ncclGetErrorString.argtypes = [C.c_int]
        L.ncclGetErrorString.restype = C.c_char_p
        self.mark = 0

    def take(self):
        """the parsed lines logged since the last take()"""
        n = self.L.fake_rccl_log_count()
        out = [parse_line(self.L.fake_rccl_log_line(i).decode()) for i in range(self.mark, n)]
        self.mark = n
        return out

    def depth(self):
        return self.L.fake_rccl_group_depth()

    def live_comms(self):
        return self.L.fake_rccl_live_comms()

    def fail_nth(self, fn, n):
        self.L.fake_rccl_fail_nth(fn.encode(), n)

    def reset(self):
        self.mark = 0
        return self.L.fake_rccl_reset()


def selfcheck(S):
    """the stand-in alone, no GPU: nothing here reaches a HIP call"""
    L = S.L
    out = {}
    out["send_outside_group"] = L.ncclSend(None, C.c_size_t(4), NCCL_FLOAT, 0, None, None)
    out["end_without_start"] = L.ncclGroupEnd()
    out["pair"] = [L.ncclGroupStart(), S.depth(), L.ncclGroupStart(), S.depth(), L.ncclGroupEnd(), S.depth(), L.ncclGroupEnd(), S.depth()]
    S.fail_nth("GroupStart", 2)
    out["fault"] = [L.ncclGroupStart(), L.ncclGroupEnd(), L.ncclGroupStart(), S.depth(), L.ncclGroupStart(), L.ncclGroupEnd(), S.depth()]
    out["strings"] = [L.ncclGetErrorString(k).decode() for k in range(8)]
    ids = []
    for _ in range(2):
        buf = C.create_string_buffer(128)
        L.ncclGetUniqueId(buf)
        ids.append(buf.raw.hex())
    out["ids"] = ids
    out["log"] = S.take()
    out["reset"] = [S.reset(), L.fake_rccl_log_count()]
    return out


def make_film(W, H, seed):
    """[H, W, 4] uint32: seeded random float32 bit patterns in all four channels, with NaN payloads and -0.0 planted"""
    rng = np.random.RandomState(seed)
    film = rng.randint(0, 2 ** 32, (H, W, 4), dtype=np.uint64).astype(np.uint32)
    flat = film.reshape(-1)
    special = np.array([0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001, 0x00000000], np.uint32)
    where = rng.permutation(flat.size)[:min(flat.size, 2 * special.size)]
    flat[where] = np.resize(special, where.size)
    return film


def compact_of(film, tiles, H, W, block, world, rank):
    """the rank's compact buffer [max_local_rows, W, 4] by the inverse row-block mapping (test_tiles.test_deinterleave_roundtrip), the rows
    past its share holding the sentinel"""
    b = np.full((tiles.max_local_rows(H, world, block), W, 4), SENTINEL, np.uint32)
    for (y0, h, off) in tiles.row_blocks(H, rank, world, block):
        b[off:off + h] = film[H - y0 - h:H - y0]
    return b


def film_report(got, film):
    differ = (got != film).any(-1)
    return {"exact": got.tobytes() == film.tobytes(), "pixels_differing": int(differ.sum()), "pixels_still_ff": int((got == 0xFFFFFFFF).all(-1).sum())}


class Ranks:
    """world contexts (each on a non-blocking stream of its own if streams) and their communicators on one fresh id"""

    def __init__(self, ag, S, world, streams=False):
        self.ag, self.S, self.world = ag, S, world
        self.ctxs, self.comms, self.streams = [], [], []
        self.hip = None
        if streams:
            import hip_runtime
            self.hip = hip_runtime.runtime()      # (asserts that the stand-in and the library share one HIP runtime)
            self.streams = [self.hip.stream_create() for _ in range(world)]
        uid = ag.comm_unique_id()
        for r in range(world):
            self.ctxs.append(ag.Context(0, stream=self.streams[r] if streams else None))
            self.comms.append(ag.Comm(self.ctxs[r], world, r, unique_id=uid))
        self.opened = S.take()

    def close(self):
        """-> the lines the closes logged"""
        self.S.take()
        for m in self.comms:
            m.close()
        lines = self.S.take()
        for c in self.ctxs:
            c.close()
        for s in self.streams:
            self.hip.stream_destroy(s)
        return lines

    def raw_gather(self, r, local, W, H, block, full):
        """agpt_gather_tiles of rank r without the binding's exception -> (status, message)"""
        L = self.ctxs[r].L
        rc = L.agpt_gather_tiles(self.comms[r].h, C.c_void_p(local), W, H, block, C.c_void_p(full) if full else None)
        return rc, L.agpt_last_error().decode() if rc else ""

    def gather(self, W, H, block, seed, tiles, stop_after=None, before=None, order=None, delay=None):
        """One gather of a fresh random film through Comm.gather_tiles, the peers first (or the ranks of `order`).  before(rank) runs just
        ahead of each rank's call; stop_after: that rank's call goes through raw_gather and is the last.  delay (a hip_runtime.Delay, with
        streams): every rank's compact buffer holds finite wrong values, and only a copy enqueued on the rank's stream behind the delay,
        which the host does not wait for, puts the real ones there (test_gpu_streams.py's pattern); "busy" is hipStreamQuery of the
        rank's stream just ahead of its call.  -> the record of the JSON"""
        film = make_film(W, H, seed)
        world, ctxs = self.world, self.ctxs
        rec = {"W": W, "H": H, "block": block, "world": world, "calls": {}, "depth": {}, "status": {}}
        locals_, reals = [], []
        full = ctxs[0].alloc(W * H * 16)
        try:
            ctxs[0].memset(full, 0xFF, W * H * 16)
            for r in range(world):
                host = compact_of(film, tiles, H, W, block, world, r)
                locals_.append(ctxs[r].alloc(host.nbytes))
                if delay is None:
                    ctxs[r].upload(locals_[r], host)
                else:
                    ctxs[r].memset(locals_[r], 0x5A, host.nbytes)
                    reals.append(ctxs[r].alloc(host.nbytes))
                    ctxs[r].upload(reals[r], host)
            if delay is not None:
                rec["busy"] = {}
                for r in range(world):
                    delay.enqueue(self.streams[r])
                    self.hip.copy_async(locals_[r], reals[r], host.nbytes, self.streams[r])      # (every rank's buffer has max_local_rows rows)
            self.S.take()
            for r in order or list(range(1, world)) + [0]:
                if before:
                    before(r)
                if delay is not None:
                    rec["busy"][str(r)] = self.hip.stream_query(self.streams[r])
                if r == stop_after:
                    rec["status"][str(r)] = list(self.raw_gather(r, locals_[r], W, H, block, full if r == 0 else 0))
                else:
                    self.comms[r].gather_tiles(locals_[r], W, H, block, full if r == 0 else 0)
                    rec["status"][str(r)] = [0, ""]
                rec["calls"][str(r)] = self.S.take()
                rec["depth"][str(r)] = self.S.depth()
                if r == stop_after:
                    break
            got = ctxs[0].download(full, (H, W, 4), np.uint32)      # (synchronises rank 0's stream)
            if stop_after is None:
                rec["film"] = film_report(got, film)
        finally:
            for s in self.streams:
                self.hip.stream_synchronize(s)
            for r, p in enumerate(locals_):
                ctxs[r].free(p)
            for r, p in enumerate(reals):
                ctxs[r].free(p)
            ctxs[0].free(full)
        return rec


def run_cases(ag, S, out):
    from ag_pathtracer_amd import tiles
    cases = out["cases"]

    # ---- the table ----
    for k, (W, H, block, world) in enumerate(GATHER_CASES):
        R = Ranks(ag, S, world)
        rec = R.gather(W, H, block, 100 + k, tiles)
        rec["opened"] = R.opened
        rec["closed"] = R.close()
        rec["live_comms_after"] = S.live_comms()
        cases[case_name(W, H, block, world)] = rec

    # ---- 1. one set of communicators, three shapes: the staging buffer grows, the slot size changes back ----
    R = Ranks(ag, S, 3)
    cases["regrow"] = [R.gather(W, H, 8, 200 + k, tiles) for k, (W, H) in enumerate([(5, 37), (96, 77), (5, 37)])]
    R.close()

    # ---- 2. every rank's context on a caller's non-blocking stream ----
    R = Ranks(ag, S, 3, streams=True)
    rec = R.gather(96, 77, 8, 300, tiles)
    rec["streams"] = list(R.streams)
    cases["streams"] = rec
    # ... and the compact buffers filled on those streams behind a delay: only the streams order the gather behind its inputs
    import hip_runtime
    delay = hip_runtime.Delay(R.ctxs[0], R.streams[0])
    try:
        rec = R.gather(96, 77, 8, 301, tiles, delay=delay)
    finally:
        delay.free()
    rec["streams"] = list(R.streams)
    rec["delay_ms"] = delay.ms
    cases["streams_delay"] = rec
    R.close()

    # ---- 3. end to end: three ranks render their interleaved shares of C1, the gather follows ----
    W, H, spp, world = 96, 77, 2, 3
    R = Ranks(ag, S, world)
    pt = ag.PathTracer(5)
    scenes = [ag.scenes.scene_c1().instantiate(ag.Scene(c)) for c in R.ctxs]
    rows = tiles.max_local_rows(H, world)
    ptrs = [c.alloc(rows * W * 16) for c in R.ctxs]
    full = R.ctxs[0].alloc(W * H * 16)
    try:
        ref, _ = pt.render_to_host(scenes[0], W, H, spp)
        R.ctxs[0].memset(full, 0xFF, W * H * 16)
        for r in range(world):
            R.ctxs[r].memset(ptrs[r], 0, rows * W * 16)
            pt.render(scenes[r], W, H, spp, ptrs[r], accum_pitch=W, interleave=(tiles.BLOCK_ROWS, world, r))
        for r in (1, 2, 0):
            R.comms[r].gather_tiles(ptrs[r], W, H, tiles.BLOCK_ROWS, full if r == 0 else 0)
        got = R.ctxs[0].download(full, (H, W, 4))
        same = (got[..., :3].view(np.uint32) == ref[..., :3].view(np.uint32)).all(-1)
        cases["render"] = {"exact": got[..., :3].tobytes() == ref[..., :3].tobytes(), "pixels_differing": int((~same).sum()),
                           "lit_pixels": int((ref[..., :3] > 0).any(-1).sum()), "depth": S.depth()}
    finally:
        for r in range(world):
            R.ctxs[r].free(ptrs[r])
            scenes[r].close()
        R.ctxs[0].free(full)
    R.close()

    # ---- 4. errors, each followed by a clean gather on the same communicators ----
    R = Ranks(ag, S, 3)
    faults = cases["faults"] = {}
    for k, (fn, rank) in enumerate(FAULTS):
        rec = R.gather(5, 37, 8, 400 + k, tiles, stop_after=rank, before=lambda r, fn=fn, rank=rank: S.fail_nth(fn, 1) if r == rank else None)
        S.fail_nth("", 0)
        rec["sends_left_posted"] = S.reset()
        rec["clean"] = R.gather(5, 37, 8, 450 + k, tiles)
        faults["%s@%d" % (fn, rank)] = rec
    # rank 0 alone: its receives are queued, and the group's end finds no send -- an error that only GroupEnd returns
    cases["no_sends"] = R.gather(5, 37, 8, 480, tiles, stop_after=0, order=[0])
    cases["no_sends"]["clean"] = R.gather(5, 37, 8, 481, tiles)

    # ---- 5. arguments ----
    args = cases["arguments"] = {}
    W, H, block = 5, 37, 8
    film = make_film(W, H, 500)
    host = [compact_of(film, tiles, H, W, block, 3, r) for r in range(3)]
    ptrs = [R.ctxs[r].alloc(host[r].nbytes) for r in range(3)]
    full = R.ctxs[0].alloc(W * H * 16)
    try:
        for r in range(3):
            R.ctxs[r].upload(ptrs[r], host[r])
        R.ctxs[0].memset(full, 0xFF, W * H * 16)
        S.take()
        args["rank0_null_full"] = {"status": list(R.raw_gather(0, ptrs[0], W, H, block, 0)), "calls": S.take()}
        args["peer_null_full"] = {"status": [list(R.raw_gather(r, ptrs[r], W, H, block, 0)) for r in (1, 2)], "calls": S.take()}
        args["then_rank0"] = {"status": list(R.raw_gather(0, ptrs[0], W, H, block, full)), "calls": S.take(),
                              "film": film_report(R.ctxs[0].download(full, (H, W, 4), np.uint32), film)}
        h = C.c_void_p()
        rc = R.ctxs[0].L.agpt_comm_init(R.ctxs[0].h, None, 2, 0, C.byref(h))
        args["init_null_id"] = {"status": rc, "handle": h.value, "calls": S.take()}
    finally:
        for r in range(3):
            R.ctxs[r].free(ptrs[r])
        R.ctxs[0].free(full)
    args["close"] = {"calls": R.close(), "live_comms_after": S.live_comms()}


def main(argv):
    path, out_path = argv[1], argv[2]
    t0 = time.perf_counter()
    S = StandIn(path)
    if len(argv) > 3 and argv[3] == "selfcheck":
        with open(out_path, "w") as f:
            json.dump(selfcheck(S), f)
        return 0
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ag_pathtracer_amd as ag
    uid = ag.comm_unique_id()
    lines = S.take()
    if [ln["fn"] for ln in lines] != ["GetUniqueId"] or not uid.startswith(ID_TAG):
        print("the real librccl was bound: log %s, id %s" % (lines, uid[:16]), file=sys.stderr)
        return 3
    out = {"bound": {"lines": lines, "id": uid.hex()}, "cases": {}, "exception": None}
    try:
        run_cases(ag, S, out)
    except BaseException:      # noqa: BLE001 -- nothing more is started on the GPU; what there is, is written
        out["exception"] = traceback.format_exc()
    out["torch_imported"] = "torch" in sys.modules
    out["depth_at_end"] = S.depth()
    out["seconds"] = time.perf_counter() - t0
    with open(out_path, "w") as f:
        json.dump(out, f)
    return 0 if out["exception"] is None else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
