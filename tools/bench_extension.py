#!/usr/bin/env python
"""Time the normal extension in HBM (cutfemx_amd/csrc/cfx_extend.hip) beside the reinitialisation it builds on.

    python tools/bench_extension.py --n 128 512 --out profiles

Workload: the sphere of tools/bench_reinit.py (the bench's sphere times 1 + x_0, so that it is not a distance already)
on the n^3 Kuhn box, interface speed w = 1 + x_0; at n <= 256 unbanded and with max_distance = 4 h, above that banded
only.  Every figure is the HIP-event time of one call on device tensors after one warm-up call, as the median of
--repeats runs, with the range: cutfemx_amd.distance.extend_normal_velocity (its three result tensors are allocated
inside the call and count), and cutfemx_amd.distance.reinitialize with the same options in the same session (phi restored
from a device copy before each call, outside the events).  The number to read is their ratio.

Kernel split: from a separate run under the profiler,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_extension.py --once N [--band]
    python tools/bench_extension.py --n N --out profiles --stats DIR

--once makes one extension call and nothing else; --stats folds the reinit_* and extend_* rows of DIR's
*kernel_stats.csv into the record.  One JSON file per size (extension_n<N>.json) and a table on stdout.  Nothing here
runs without a GPU."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import bench_reinit as BR  # noqa: E402

BAND_LAYERS = BR.BAND_LAYERS
UNBANDED_UP_TO = 256


def speed(torch, n, device):
    ax = torch.arange(n + 1, device=device, dtype=torch.float64) / n
    return (1.0 + ax[None, None, :]).expand(n + 1, n + 1, n + 1).reshape(-1).contiguous()


def timed(torch, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = call()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def modes_for(n):
    modes = [("band_4h", BAND_LAYERS / n)]
    return ([("unbanded", None)] if n <= UNBANDED_UP_TO else []) + modes


def run(n, repeats):
    torch, cfx, V, phi0 = BR.setup(n)
    w = speed(torch, n, phi0.device)
    phi, work = cfx.Function(V, phi0.clone()), cfx.Function(V, phi0.clone())
    result = dict(n=n, vertices=V.ndofs, cells=V.mesh.num_cells, h=1.0 / n, repeats=repeats, modes={})
    for mode, band in modes_for(n):
        kw = dict(max_distance=band, max_iter=100000)
        ext = lambda: cfx.distance.extend_normal_velocity(phi, w, **kw)

        def reinit():
            return cfx.distance.reinitialize(work, **kw)
        res, _ = timed(torch, ext)                                                        # warm-up
        info = res.info
        del res
        work.values.copy_(phi0)
        timed(torch, reinit)
        te, tr = [], []
        for _ in range(repeats):
            res, t = timed(torch, ext)
            assert res.info == info, (res.info, info)
            del res
            te.append(t)
            work.values.copy_(phi0)
            rinfo, t = timed(torch, reinit)
            assert (rinfo.sweeps, rinfo.updates) == (info.sweeps, info.updates)
            tr.append(t)
        stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
        result["modes"][mode] = dict(max_distance=band, reason=info.reason_name, sweeps=info.sweeps, seeds=info.seeds, updates=info.updates,
                                     transport_sweeps=info.transport_sweeps, transported=info.transported, extension=stat(te),
                                     reinitialize=stat(tr), ratio=statistics.median(te) / statistics.median(tr))
    return result


def once(n, band):
    torch, cfx, V, phi0 = BR.setup(n)
    res = cfx.distance.extend_normal_velocity(cfx.Function(V, phi0), speed(torch, n, phi0.device),
                                              max_distance=BAND_LAYERS / n if band else None, max_iter=100000)
    torch.cuda.synchronize()
    print(f"once n {n} band {band}: {res.info}")


def kernel_split(stats_dir):
    import csv
    rows = []
    for path in sorted(Path(stats_dir).rglob("*kernel_stats.csv")):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                for stem in ("reinit_", "extend_"):
                    if stem in name:
                        short = name[name.index(stem):].split("(")[0].split("<")[0]
                        rows.append(dict(kernel=short, calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) * 1e-6,
                                         average_us=float(r["AverageNs"]) * 1e-3))
    total = sum(r["total_ms"] for r in rows)
    for r in rows:
        r["share"] = r["total_ms"] / total if total else 0.0
    return sorted(rows, key=lambda r: -r["total_ms"])


def table(r):
    lines = [f"n = {r['n']}: {r['vertices']} vertices, {r['cells']} cells"]
    for mode, m in r["modes"].items():
        e, q = m["extension"], m["reinitialize"]
        lines.append(f"  {mode:9s}: {m['sweeps']} + {m['transport_sweeps']} sweeps, {m['transported']} transported; extension "
                     f"{e['median_ms']:.2f} ms ({e['min_ms']:.2f}-{e['max_ms']:.2f}), reinitialize {q['median_ms']:.2f} ms "
                     f"({q['min_ms']:.2f}-{q['max_ms']:.2f}), ratio {m['ratio']:.2f}")
    for k in r.get("kernel_split", []):
        lines.append(f"  {k['kernel']:22s} {k['calls']:6d} calls {k['total_ms']:10.3f} ms {100 * k['share']:5.1f} % ({k['average_us']:.1f} us each)")
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
        sys.exit("bench_extension: no GPU (nothing here is measured without one)")
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
        (out / f"extension_n{n}.json").write_text(json.dumps(r, indent=1) + "\n")
        print(table(r), flush=True)


if __name__ == "__main__":
    main()
