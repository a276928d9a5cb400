"""Query-selection benchmark (separate from bench.py): ChunkStore.query against what a DN
has without it.

Workload: a 1-D table of 16-byte records (id i8, val i4, px f4) in chunks of 65536 rows --
256 chunks of 1 MiB, all resident in the HBM cache -- and the query `(val < K) & (px >= 0.0)`
with K chosen for 0.1 %, 10 % and 100 % of the rows.  Reported, each as the median of repeated
runs after a warm-up (the variants of one comparison alternate inside one loop):

  mask / emit kernels   HIP events around LAUNCHES back-to-back hsds_query_mask (and
                        hsds_query_emit) calls, divided by their number, in rows/s and bytes/s
  query                 host to host: the query text -> response rows in host memory
                        (host clock, ending in the device-to-host copy of the rows)
  baseline              what a data node has at the parent commit: get_chunks for the
                        chunks, ONE device copy that packs them and ONE device-to-host copy
                        into a page-locked buffer allocated beforehand, then numpy evaluating
                        the same expression per chunk and building the same response records

Every variant's rows are compared with numpy over the table's closed form before it is timed.
Usage: python tools/bench_query.py [--out profiles/query_bench.json] [--reps N]"""
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
DT = np.dtype([("id", "<i8"), ("val", "<i4"), ("px", "<f4")])
CHUNK, NCHUNKS = 65536, 256
NROWS = CHUNK * NCHUNKS
LAUNCHES = 20
SELECTIVITY = {"0.1%": 1, "10%": 100, "100%": 1000}


def chunk_rows(i):
    """the table's closed form: val cycles through 0..999 in a scrambled order"""
    r = np.arange(i * CHUNK, (i + 1) * CHUNK, dtype=np.int64)
    a = np.zeros(CHUNK, DT)
    a["id"] = r
    a["val"] = (r * 7919) % 1000
    a["px"] = (r % 4096).astype(np.float32) * 0.25
    return a


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "clk" in ln.lower()]
    except Exception as e:          # noqa: BLE001 - context only
        return [f"unavailable: {e}"]


def stat(v):
    return {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import torch
    from hsds_amd import query as qry
    from hsds_amd.datanode import ChunkRead, ChunkStore
    from hsds_amd.partition import getS3Key
    assert torch.cuda.is_available(), "bench_query needs a GPU"
    dev = torch.device("cuda", 0)
    ids = [f"c-{DSET[2:]}_{i}" for i in range(NCHUNKS)]
    keys = {getS3Key(cid): i for i, cid in enumerate(ids)}
    store = ChunkStore(lambda k, o, ln: chunk_rows(keys[k]).tobytes(), mem_target=1 << 30, device=dev)
    eng = store.reader.eng
    reads = [ChunkRead(cid, getS3Key(cid)) for cid in ids]
    store.get_chunks(reads, DT, (CHUNK,))              # every chunk resident
    assert len(store.cache) == NCHUNKS
    table = np.concatenate([chunk_rows(i) for i in range(NCHUNKS)])
    segs, rsp_dt = qry.query_segments(DT)
    pinned = torch.empty((NCHUNKS, CHUNK * DT.itemsize), dtype=torch.uint8, pin_memory=True)
    result = {"workload": {"rows": NROWS, "record_bytes": DT.itemsize, "chunk_rows": CHUNK, "chunks_resident": NCHUNKS,
                           "response_record_bytes": rsp_dt.itemsize, "reps": args.reps, "statistic": "median"},
              "device": torch.cuda.get_device_name(0), "clocks_before": clocks(), "sets": {},
              "method": {"kernels": f"HIP events around {LAUNCHES} back-to-back launches, divided by {LAUNCHES}",
                         "host_to_host": "host clock from the query text to response rows in host memory",
                         "baseline": "get_chunks, one packing copy on the device, one device-to-host copy into "
                                     "page-locked memory allocated beforehand, numpy evaluating the expression "
                                     "per chunk and building the response records"}}

    def expected(k):
        hits = np.nonzero((table["val"] < k) & (table["px"] >= 0.0))[0]
        out = np.zeros(len(hits), rsp_dt)
        out["index"] = hits
        for f in DT.names:
            out[f] = table[f][hits]
        return out

    def run_query(text):
        res = store.query(DSET, (NROWS,), (CHUNK,), None, text, DT)
        return res.rows.cpu().numpy().view(rsp_dt)

    def baseline(text):
        expr = qry.eval_str(qry.parse(text), "rows")
        vals = store.get_chunks(reads, DT, (CHUNK,))
        pinned.copy_(torch.stack([v.view(torch.uint8).reshape(-1) for v in vals]))
        host = pinned.numpy()
        parts = []
        for i in range(NCHUNKS):
            rows = host[i].view(DT)
            hits = np.nonzero(eval(expr, {}, {"rows": rows}))[0]
            rec = np.zeros(len(hits), rsp_dt)
            rec["index"] = hits + i * CHUNK
            for f in DT.names:
                rec[f] = rows[f][hits]
            parts.append(rec)
        return np.concatenate(parts)

    abase = store.cache.arena.buf
    chunks = [(store.cache._lru[cid].off, 0, CHUNK, 1, i * CHUNK) for i, cid in enumerate(ids)]
    tab, nwords = qry.query_chunk_table(chunks)
    d_tab = torch.from_numpy(tab.view(np.int64).reshape(-1)).to(dev)
    mask = torch.empty(nwords, dtype=torch.int64, device=dev)
    count = torch.empty(nwords, dtype=torch.int32, device=dev)
    for name, k in SELECTIVITY.items():
        text = f"(val < {k}) & (px >= 0.0)"
        want = expected(k)
        for _ in range(2):                                   # correctness of every variant first (also the warm-up)
            assert run_query(text).tobytes() == want.tobytes()
            assert baseline(text).tobytes() == want.tobytes()
        cq = qry.compile_query(text, DT)
        eng.query_mask(abase, d_tab, NCHUNKS, nwords, DT.itemsize, cq.prog, None, mask, count)
        incl = torch.cumsum(count, 0, dtype=torch.int64)
        base = incl - count
        total = int(incl[-1])
        assert total == len(want)
        out = torch.empty(total * rsp_dt.itemsize, dtype=torch.uint8, device=dev)
        eng.query_emit(abase, d_tab, NCHUNKS, nwords, DT.itemsize, mask, base, 0, segs, rsp_dt.itemsize, out)
        assert out.cpu().numpy().tobytes() == want.tobytes()
        times = {"mask": [], "emit": [], "scan": []}
        for rep in range(args.reps + 3):
            for which in times:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(LAUNCHES):
                    if which == "mask":
                        eng.query_mask(abase, d_tab, NCHUNKS, nwords, DT.itemsize, cq.prog, None, mask, count)
                    elif which == "emit":
                        eng.query_emit(abase, d_tab, NCHUNKS, nwords, DT.itemsize, mask, base, 0, segs,
                                       rsp_dt.itemsize, out)
                    else:
                        torch.cumsum(count, 0, dtype=torch.int64)
                b.record()
                b.synchronize()
                if rep >= 3:
                    times[which].append(a.elapsed_time(b) / LAUNCHES)
        kern = {w: stat(v) for w, v in times.items()}
        kern["mask"]["rows_per_s"] = round(NROWS / (kern["mask"]["ms"] * 1e-3))
        kern["mask"]["read_bytes_per_s"] = round(NROWS * DT.itemsize / (kern["mask"]["ms"] * 1e-3))
        kern["emit"]["response_bytes_per_s"] = round(total * rsp_dt.itemsize / (kern["emit"]["ms"] * 1e-3))
        h2h = {"query": [], "baseline_get_chunks_d2h_numpy": []}
        for rep in range(args.reps):
            for key, fn in (("query", lambda: run_query(text)), ("baseline_get_chunks_d2h_numpy", lambda: baseline(text))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                h2h[key].append((time.perf_counter() - t0) * 1e3)
        result["sets"][name] = {"query": text, "rows_matched": total, "kernels": kern,
                                "host_to_host_ms": {key: stat(v) for key, v in h2h.items()},
                                "baseline_d2h_bytes": NROWS * DT.itemsize, "answer_bytes": total * rsp_dt.itemsize}
    result["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
