"""Point-selection benchmark (separate from bench.py): ChunkStore.get_points against what a
DN can do without it.

Workload: an 8192 x 8192 f32 dataset in 512 x 512 chunks -- 256 chunks of 1 MiB, all
resident in the HBM cache -- and two sets of 1 M points: uniformly random over the
dataset, and drawn from 16 of the chunks.  Reported, each as the median of repeated runs
after a warm-up (the variants of one comparison alternate inside one loop):

  gather kernel alone   HIP events around LAUNCHES back-to-back hsds_points_gather calls,
                        divided by their number (one launch between two events is mostly
                        the host's launch gap), in points/s and output bytes/s: request
                        order with a contiguous output, and points pre-sorted by (chunk,
                        offset) with a scattered dst_index, plus what the sort itself costs
  get_points            host to host: points in host memory -> values in host memory
                        (host clock, ending in the device-to-host copy)
  baseline              the same request with get_chunks for the touched chunks, ONE
                        device copy that packs them and ONE device-to-host copy into a
                        page-locked buffer allocated beforehand (the kindest form of it),
                        and numpy fancy indexing
  numpy only            fancy indexing with the chunks already in host memory (context:
                        the reference's best case, kinder than its per-point loop)

Every variant's values are compared with the dataset's closed form before it is timed.
Usage: python tools/bench_points.py [--out profiles/points_bench.json] [--points N]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DSET = "d-0f1e2d3c-4b5a6978-8796-a5b4c3-d2e1f0a9b8"
DIMS, LAYOUT = (8192, 8192), (512, 512)
DT = np.dtype("<f4")
LAUNCHES = 50            # gather launches between two events


def value_at(r, c):
    """the dataset's closed form (exact in f32)"""
    return ((r.astype(np.int64) * 8192 + c.astype(np.int64)) % (1 << 24)).astype(DT)


def chunk_bytes(i, j):
    r = np.arange(i * 512, (i + 1) * 512, dtype=np.int64)
    c = np.arange(j * 512, (j + 1) * 512, dtype=np.int64)
    return ((r[:, None] * 8192 + c[None, :]) % (1 << 24)).astype(DT).tobytes()


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "clk" in ln.lower()]
    except Exception as e:          # noqa: BLE001 - context only
        return [f"unavailable: {e}"]


def median_ms(samples):
    return round(statistics.median(samples), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_bench.json"))
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    import torch
    from hsds_amd.datanode import ChunkRead, ChunkStore
    from hsds_amd.partition import getS3Key
    assert torch.cuda.is_available(), "bench_points needs a GPU"
    dev = torch.device("cuda", 0)
    n = args.points
    keys = {}
    for i in range(16):
        for j in range(16):
            keys[getS3Key(f"c-{DSET[2:]}_{i}_{j}")] = (i, j)
    store = ChunkStore(lambda k, o, ln: chunk_bytes(*keys[k]), mem_target=1 << 30, device=dev)
    eng = store.reader.eng
    rng = np.random.default_rng(1)
    uniform = np.stack([rng.integers(0, 8192, n), rng.integers(0, 8192, n)], axis=1).astype(np.uint64)
    hot = rng.choice(256, 16, replace=False)
    pick = hot[rng.integers(0, 16, n)]
    clustered = np.stack([(pick // 16) * 512 + rng.integers(0, 512, n), (pick % 16) * 512 + rng.integers(0, 512, n)],
                         axis=1).astype(np.uint64)
    allreads = [ChunkRead(f"c-{DSET[2:]}_{i}_{j}", getS3Key(f"c-{DSET[2:]}_{i}_{j}")) for i in range(16)
                for j in range(16)]
    store.get_chunks(allreads, DT, LAYOUT)              # every chunk resident
    assert len(store.cache) == 256
    host_chunks = np.stack([np.frombuffer(chunk_bytes(i, j), DT).reshape(LAYOUT) for i in range(16)
                            for j in range(16)])
    result = {"workload": {"dataset": list(DIMS), "layout": list(LAYOUT), "dtype": "f4", "chunks_resident": 256,
                           "points": n, "reps": args.reps, "statistic": "median"},
              "device": torch.cuda.get_device_name(0), "clocks_before": clocks(), "sets": {},
              "method": {"gather_kernel": f"HIP events around {LAUNCHES} back-to-back launches, divided by {LAUNCHES}",
                         "host_to_host": "host clock from points in host memory to values in host memory",
                         "baseline": "get_chunks, one packing copy on the device, one device-to-host copy into "
                                     "page-locked memory allocated beforehand, numpy fancy indexing"}}
    pinned = torch.empty((256,) + LAYOUT, dtype=torch.float32, pin_memory=True)

    def baseline(pts):
        p = pts.astype(np.int64)
        ci = p // 512
        uniq, inv = np.unique(ci[:, 0] * 16 + ci[:, 1], return_inverse=True)
        reads = [allreads[k] for k in uniq]
        vals = store.get_chunks(reads, DT, LAYOUT)
        host = pinned[:len(vals)]
        host.copy_(torch.stack(vals))
        host = host.numpy()
        return host[inv, p[:, 0] - ci[:, 0] * 512, p[:, 1] - ci[:, 1] * 512], len(uniq)

    def numpy_only(pts):
        p = pts.astype(np.int64)
        ci = p // 512
        return host_chunks[ci[:, 0] * 16 + ci[:, 1], p[:, 0] - ci[:, 0] * 512, p[:, 1] - ci[:, 1] * 512]

    def get_points(pts):
        return store.get_points(DSET, DIMS, LAYOUT, pts, DT).cpu().numpy().view(DT)

    for name, pts in (("uniform", uniform), ("clustered16", clustered)):
        want = value_at(pts[:, 0], pts[:, 1])
        # ---- correctness of every variant first (also the warm-up)
        for _ in range(2):
            got_b, touched = baseline(pts)
            assert np.array_equal(got_b, want)
            assert np.array_equal(numpy_only(pts), want)
            assert np.array_equal(get_points(pts), want)
        # ---- the gather kernel alone
        d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
        chunk, eoff, _ = eng.locate_points(d_pts, DIMS, LAYOUT, 4)
        uniq, which = torch.unique(chunk, return_inverse=True)
        abase = store.cache.arena.buf
        slot = torch.tensor([store.cache._lru[allreads[int(k)].chunk_id].off for k in uniq.cpu().numpy()],
                            dtype=torch.int64, device=dev)
        order = torch.sort(which * (1 << 20) + eoff)[1]
        which_s, eoff_s = which[order].contiguous(), eoff[order].contiguous()
        out = torch.empty(n * 4, dtype=torch.uint8, device=dev)
        segs = [(0, 0, 4)]
        variants = {"request_order_contiguous": (which, eoff, None), "presorted_scattered": (which_s, eoff_s, order)}
        for w, e, di in variants.values():
            out.zero_()
            eng.gather_points(abase, slot, w, e, segs, 4, 4, out, dst_index=di)
            assert np.array_equal(out.cpu().numpy().view(DT), want)
        times = {k: [] for k in variants}
        sort_ms = []
        for rep in range(args.reps + 3):
            for k, (w, e, di) in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(LAUNCHES):
                    eng.gather_points(abase, slot, w, e, segs, 4, 4, out, dst_index=di)
                b.record()
                b.synchronize()
                if rep >= 3:
                    times[k].append(a.elapsed_time(b) / LAUNCHES)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            o2 = torch.sort(which * (1 << 20) + eoff)[1]
            _ = which[o2], eoff[o2]
            b.record()
            b.synchronize()
            if rep >= 3:
                sort_ms.append(a.elapsed_time(b))
        kern = {}
        for k, ts in times.items():
            ms = median_ms(ts)
            kern[k] = {"ms": ms, "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                       "points_per_s": round(n / (ms * 1e-3)), "output_bytes_per_s": round(4 * n / (ms * 1e-3))}
        kern["presort_cost_ms"] = median_ms(sort_ms)          # the sort and the two index gathers it needs
        # ---- host to host, alternating
        h2h = {"get_points": [], "baseline_get_chunks_d2h_numpy": [], "numpy_only_chunks_in_host_memory": []}
        for rep in range(args.reps):
            for k, fn in (("get_points", lambda: get_points(pts)),
                          ("baseline_get_chunks_d2h_numpy", lambda: baseline(pts)),
                          ("numpy_only_chunks_in_host_memory", lambda: numpy_only(pts))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                h2h[k].append((time.perf_counter() - t0) * 1e3)
        result["sets"][name] = {
            "chunks_touched": touched, "gather_kernel": kern,
            "host_to_host_ms": {k: {"ms": median_ms(v), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                                for k, v in h2h.items()},
            "baseline_d2h_bytes": touched << 20, "answer_bytes": 4 * n}
    result["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
