#!/usr/bin/env python
"""Time the reinitialisation in HBM (cutfemx_amd/csrc/cfx_reinit.hip) on the sphere of bench.py.

    python tools/bench_reinit.py --n 128 512 --out profiles

Workload: the bench's sphere level set multiplied by (1 + x_0), so that it is not a distance already, on the n^3 Kuhn
box; unbanded and with max_distance = 4 h.  Every figure is the HIP-event time of one cutfemx_amd.distance.reinitialize
call on a device tensor (restored from a device copy before each call, outside the events) after one warm-up call, as the
median of --repeats runs, with the range.  Two cadences: the default (the host looks every 8 sweeps) and "quiet"
(check_every = 0, device info, exactly as many sweeps launched as the first run needed: no host round trip).
Fields: sweeps, seeds, updates, updates per second and time per sweep.

Kernel split: from a separate run under the profiler,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_reinit.py --once N [--band]
    python tools/bench_reinit.py --n N --out profiles --stats DIR

--once makes one call and nothing else; --stats folds the reinit_* rows of DIR's *kernel_stats.csv into the record.
One JSON file per size (reinit_n<N>.json) and a table on stdout.  Nothing here runs without a GPU."""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BAND_LAYERS = 4


def level_set(torch, n, device):
    ax = torch.arange(n + 1, device=device, dtype=torch.float64) / n
    cx, cy, cz, R = 0.47, 0.43, 0.41, 0.31
    d2 = (ax[:, None, None] - cz) ** 2 + (ax[None, :, None] - cy) ** 2 + (ax[None, None, :] - cx) ** 2
    return ((torch.sqrt(d2) - R) * (1.0 + ax[None, None, :])).reshape(-1).contiguous()


def setup(n):
    import torch

    import cutfemx_amd as cfx
    device = torch.device("cuda", torch.cuda.current_device())
    mesh = cfx.Mesh.create_box(3, n)
    V = cfx.FunctionSpace(mesh, 1)
    phi0 = level_set(torch, n, device)
    return torch, cfx, V, phi0


def timed_call(torch, cfx, fn, phi0, **kw):
    fn.values.copy_(phi0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    info = cfx.distance.reinitialize(fn, **kw)
    b.record()
    torch.cuda.synchronize()
    return info, a.elapsed_time(b)


def run(n, repeats):
    torch, cfx, V, phi0 = setup(n)
    fn = cfx.Function(V, phi0.clone())
    result = dict(n=n, vertices=V.ndofs, cells=V.mesh.num_cells, h=1.0 / n, repeats=repeats, modes={})
    for mode, band in (("unbanded", None), ("band_4h", BAND_LAYERS / n)):
        info, _ = timed_call(torch, cfx, fn, phi0, max_distance=band, max_iter=100000)       # warm-up
        buf = cfx.distance.reinit_info_buffer()
        loud, quiet = [], []
        for _ in range(repeats):
            i1, t = timed_call(torch, cfx, fn, phi0, max_distance=band, max_iter=100000)
            loud.append(t)
            _, t = timed_call(torch, cfx, fn, phi0, max_distance=band, max_iter=info.sweeps, check_every=0, info_out=buf)
            quiet.append(t)
            i2 = cfx.distance.read_reinit_info(buf)
            assert i1 == info and i2 == info, (info, i1, i2)
        stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
        ms = statistics.median(quiet)
        result["modes"][mode] = dict(max_distance=band, reason=info.reason_name, sweeps=info.sweeps, seeds=info.seeds,
                                     updates=info.updates, check_every_8=stat(loud), quiet=stat(quiet),
                                     updates_per_second=info.updates / (ms * 1e-3), us_per_sweep=1e3 * ms / max(info.sweeps, 1),
                                     updates_per_vertex=info.updates / V.ndofs)
    return result


def once(n, band):
    torch, cfx, V, phi0 = setup(n)
    fn = cfx.Function(V, phi0)
    info = cfx.distance.reinitialize(fn, max_distance=BAND_LAYERS / n if band else None, max_iter=100000)
    torch.cuda.synchronize()
    print(f"once n {n} band {band}: {info}")


def kernel_split(stats_dir):
    rows = []
    for path in sorted(Path(stats_dir).rglob("*kernel_stats.csv")):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                if "reinit_" in name:
                    short = name[name.index("reinit_"):].split("(")[0].split("<")[0]
                    rows.append(dict(kernel=short, calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) * 1e-6,
                                     average_us=float(r["AverageNs"]) * 1e-3))
    total = sum(r["total_ms"] for r in rows)
    for r in rows:
        r["share"] = r["total_ms"] / total if total else 0.0
    return sorted(rows, key=lambda r: -r["total_ms"])


def table(r):
    lines = [f"n = {r['n']}: {r['vertices']} vertices, {r['cells']} cells"]
    for mode, m in r["modes"].items():
        q, l = m["quiet"], m["check_every_8"]
        lines.append(f"  {mode:9s}: {m['sweeps']} sweeps, {m['seeds']} seeds, {m['updates']} updates "
                     f"({m['updates_per_vertex']:.2f} per vertex); quiet {q['median_ms']:.2f} ms ({q['min_ms']:.2f}-{q['max_ms']:.2f}), "
                     f"check_every 8 {l['median_ms']:.2f} ms ({l['min_ms']:.2f}-{l['max_ms']:.2f}); "
                     f"{m['updates_per_second'] / 1e9:.3f} G updates/s, {m['us_per_sweep']:.1f} us per sweep")
    for k in r.get("kernel_split", []):
        lines.append(f"  {k['kernel']:22s} {k['calls']:6d} calls {k['total_ms']:10.3f} ms {100 * k['share']:5.1f} % "
                     f"({k['average_us']:.1f} us each)")
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, nargs="+", default=[128, 512])
    p.add_argument("--repeats", type=int, default=5, help="timed runs per figure (at least 5)")
    p.add_argument("--out", default=str(ROOT / "profiles"))
    p.add_argument("--once", type=int, default=0, metavar="N", help="one call on the N^3 box and nothing else (for the profiler)")
    p.add_argument("--band", action="store_true", help="with --once: max_distance = 4 h")
    p.add_argument("--stats", default=None, metavar="DIR", help="fold the kernel stats of a profiler run into the record")
    args = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_reinit: no GPU (nothing here is measured without one)")
    if args.once:
        once(args.once, args.band)
        return
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    for n in args.n:
        r = run(n, max(args.repeats, 5))
        if args.stats:
            r["kernel_split"] = kernel_split(args.stats)
            r["kernel_split_run"] = "one unbanded call under rocprofv3 --kernel-trace --stats"
        (out / f"reinit_n{n}.json").write_text(json.dumps(r, indent=1) + "\n")
        print(table(r), flush=True)


if __name__ == "__main__":
    main()
