#!/usr/bin/env python
"""Time the semi-Lagrangian advection in HBM (cutfemx_amd/csrc/cfx_advect.hip) beside the reinitialisation that follows
it in a moving-domain loop.

    python tools/bench_advect.py --n 128 512 --out profiles

Workload: the sphere of tools/bench_reinit.py on the n^3 Kuhn box.  phi is the signed distance and the velocity is the
`velocity` that cutfemx_amd.distance.extend_normal_velocity returns for the interface speed 1 -- the unit normal field --
so that advect sees what the loop hands it.  Two modes: unbanded, and max_distance = 4 h (the extension and the
reinitialisation get the same band; advect gets one a hair below it, because both clamp to exactly the band and advect
skips |phi| > its band).  Above 256^3 the unbanded extension is not run (its workspace and its 400 sweeps serve
no purpose here): the unbanded velocity is then the sphere's analytic unit normal, and the record says so.  Two time steps:
dt = 0.5 h and 2 h (the speed is 1, so these are the CFL numbers).

Every figure is the HIP-event time of one call on device tensors after one warm-up call, as the median of --repeats runs,
with the range: cutfemx_amd.distance.advect in place on a copy of phi (restored before each call, outside the events) with
a device info, and cutfemx_amd.distance.reinitialize with the same band in the same session.  Beside the times: the
crossings (`steps`) and the longest walk, the first-use cost of the mesh's cell -> cell table (the events around the first
cfx_mesh_cell_neighbours, the vertex -> cells incidence already built) with its size, and the time against a streaming
floor at 6.3 TB/s, the copy rate measured on this GPU: nv x 64 B unbanded (phi, x, velocity, out), nv x 8 B plus 56 B per
vertex inside the band when banded.  The in-place call also copies its workspace over phi (16 B per vertex more); the
floor does not count it.

Each size runs in a process of its own under a time limit (--limit seconds); a size that fails or runs out of time ends the
tool.  One JSON file per size (advect_n<N>.json) and a table on stdout.  Nothing here runs without a GPU."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import bench_reinit as BR  # noqa: E402

BAND_LAYERS = BR.BAND_LAYERS
UNBANDED_EXTENSION_UP_TO = 256
CFLS = (0.5, 2.0)
STREAM_BYTES_PER_SECOND = 6.3e12


def timed(torch, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = call()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def analytic_normal(torch, n, device):
    ax = torch.arange(n + 1, device=device, dtype=torch.float64) / n
    cx, cy, cz = 0.47, 0.43, 0.41
    shape = (n + 1, n + 1, n + 1)
    d = torch.stack([(ax[None, None, :] - cx).expand(shape), (ax[None, :, None] - cy).expand(shape), (ax[:, None, None] - cz).expand(shape)], dim=-1)
    return (d / torch.linalg.norm(d, dim=-1, keepdim=True)).reshape(-1).contiguous()


def run(n, repeats):
    from cutfemx_amd import _lib
    torch, cfx, V, phi0 = BR.setup(n)
    nv, h = V.ndofs, 1.0 / n
    ones = torch.ones(nv, dtype=torch.float64, device=phi0.device)
    result = dict(n=n, vertices=nv, cells=V.mesh.num_cells, h=h, repeats=repeats, stream_bytes_per_second=STREAM_BYTES_PER_SECOND, modes={})
    table_ms = None
    for mode, band in (("unbanded", None), ("band_4h", BAND_LAYERS * h)):
        if band is None and n > UNBANDED_EXTENSION_UP_TO:
            dist = cfx.Function(V, phi0.clone())
            cfx.distance.reinitialize(dist, max_distance=16 * h, max_iter=100000)     # (a distance near the contour; the rest clamped)
            phi_in, vel, source = dist.values, analytic_normal(torch, n, phi0.device), "analytic unit normal of the sphere"
            del dist
        else:
            res = cfx.distance.extend_normal_velocity(cfx.Function(V, phi0), ones, max_distance=band, max_iter=100000)
            phi_in, vel, source = res.signed_distance.values, res.velocity.values, "extend_normal_velocity, speed 1"
            del res
        if table_ms is None:       # the first use of the table: the incidence it is built from exists by now
            p = C.c_void_p()
            _, table_ms = timed(torch, lambda: _lib.check(_lib.lib().cfx_mesh_cell_neighbours(V.mesh._h, C.byref(p))))
            result["cell_neighbours"] = dict(first_use_ms=table_ms, bytes=4 * 4 * V.mesh.num_cells,
                                             static_table_bytes=V.static_table_bytes()["cell_neighbours"])
        # (reinitialize and the extension clamp to exactly B, and advect skips |phi| > its own band: a band just below B skips
        # the clamped vertices)
        aband = None if band is None else band * (1.0 - 1e-9)
        inside = nv if band is None else int(torch.count_nonzero(phi_in.abs() <= aband))
        floor_bytes = 64 * nv if band is None else 8 * nv + 56 * inside
        floor_ms = 1e3 * floor_bytes / STREAM_BYTES_PER_SECOND
        work, rwork = cfx.Function(V, phi_in.clone()), cfx.Function(V, phi0.clone())
        buf = cfx.distance.advect_info_buffer()
        record = dict(max_distance=band, advect_max_distance=aband, velocity=source, vertices_in_band=inside, floor_bytes=floor_bytes, floor_ms=floor_ms, steps={})
        rkw = dict(max_distance=band, max_iter=100000)
        timed(torch, lambda: cfx.distance.reinitialize(rwork, **rkw))                 # warm-up
        tr = []
        for cfl in CFLS:
            dt = cfl * h
            adv = lambda: cfx.distance.advect(work, vel, dt, max_distance=aband, info_out=buf)
            timed(torch, adv)                                                         # warm-up
            info = cfx.distance.read_advect_info(buf)
            ta = []
            for _ in range(repeats):
                work.values.copy_(phi_in)
                _, t = timed(torch, adv)
                assert cfx.distance.read_advect_info(buf) == info
                ta.append(t)
                rwork.values.copy_(phi0)
                _, t = timed(torch, lambda: cfx.distance.reinitialize(rwork, **rkw))
                tr.append(t)
            stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
            med = statistics.median(ta)
            record["steps"][f"dt_{cfl}h"] = dict(dt=dt, located=info.located, outside=info.outside, capped=info.capped, skipped=info.skipped,
                                                 crossings=info.steps, max_walk=info.max_walk, advect=stat(ta), times_floor=med / floor_ms,
                                                 ns_per_walked_vertex=1e6 * med / max(info.located + info.outside, 1))
        record["reinitialize"] = dict(median_ms=statistics.median(tr), min_ms=min(tr), max_ms=max(tr))
        for s in record["steps"].values():
            s["share_of_reinitialize"] = s["advect"]["median_ms"] / record["reinitialize"]["median_ms"]
        result["modes"][mode] = record
        del work, rwork, vel, phi_in
    return result


def table(r):
    t = r["cell_neighbours"]
    lines = [f"n = {r['n']}: {r['vertices']} vertices, {r['cells']} cells; cell -> cell table {t['bytes'] / 1e6:.1f} MB, first use {t['first_use_ms']:.2f} ms"]
    for mode, m in r["modes"].items():
        q = m["reinitialize"]
        for name, s in m["steps"].items():
            a = s["advect"]
            lines.append(f"  {mode:9s} {name:8s}: advect {a['median_ms']:.3f} ms ({a['min_ms']:.3f}-{a['max_ms']:.3f}) = {s['times_floor']:.1f} x the floor of "
                         f"{m['floor_ms']:.3f} ms; {s['crossings']} crossings, longest walk {s['max_walk']}, outside {s['outside']}, skipped {s['skipped']}; "
                         f"reinitialize {q['median_ms']:.2f} ms ({q['min_ms']:.2f}-{q['max_ms']:.2f}): {100 * s['share_of_reinitialize']:.1f} %")
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, nargs="+", default=[128, 512])
    p.add_argument("--repeats", type=int, default=5, help="timed runs per figure (at least 5)")
    p.add_argument("--out", default=str(ROOT / "profiles"))
    p.add_argument("--limit", type=int, default=420, help="time limit of one size, seconds")
    p.add_argument("--one", type=int, default=0, metavar="N", help="run the size N in this process (what the tool starts per size)")
    args = p.parse_args()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    if args.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_advect: no GPU (nothing here is measured without one)")
        r = run(args.one, max(args.repeats, 5))
        (out / f"advect_n{args.one}.json").write_text(json.dumps(r, indent=1) + "\n")
        print(table(r), flush=True)
        return
    for n in args.n:      # each size a fresh process under its own limit; the first one that fails ends the tool
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(Path(__file__).resolve()), "--one", str(n), "--repeats", str(args.repeats),
               "--out", str(out)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"bench_advect: n = {n} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
