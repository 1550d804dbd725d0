#!/usr/bin/env python
"""Time MINRES in HBM (cutfemx_amd/csrc/cfx_solve.hip, cfx_minres_solve) on the cut Stokes system of stokes.build_blocks.

    python tools/bench_minres.py --n 128 --out profiles

The P1 vector x P1 system on Mesh.create_box(3, n) with the sphere level set of bench.py is assembled, deactivated and
merged on the GPU (stokes.assemble), then:

  ms per MINRES iteration   minres_solve over the ACTIVE rows of both blocks, check_every = 0 and rtol = 0, for two
                            iteration counts; the difference removes the set-up launches
  ms per CG iteration       cg_solve on the SAME matrix arrays.  CG breaks down on the indefinite matrix, so it is timed
                            with max_iter fixed, check_every = 0 and rtol = 0 over the active VELOCITY rows alone (that
                            block is positive definite; p stays 0 on the pressure columns); MINRES is timed on that row
                            list as well, which is the like-for-like pair
  bytes per iteration       12 nnz + 8 (rows + 1) + 16 rows for the product (tools/bench_solve.py's count) plus the vector
                            launches: 116 B per iterated row for MINRES (minres_lanczos 40, minres_update 76), 96 B for CG
                            (cg_update 60, cg_direction 36), and that figure over the time as a fraction of the 6.3 TB/s a
                            streaming kernel reaches on the MI355X
  prediction                ms per CG iteration x (MINRES bytes / CG bytes) on the velocity rows: what MINRES should take if
                            it follows its byte count as CG does
  the whole solve           minres_solve to rtol = 1e-8 over the active rows: iterations, ms, reason

Batches end in a device synchronisation; median (min - max) of `--repeats` batches, the three solvers taking turns batch
by batch.  One JSON file per size (minres_n<N>.json) and a table on stdout; nothing here runs without a GPU."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

STREAM_TBS = 6.3   # achievable HBM streaming rate of the MI355X, TB/s
MINRES_VECTOR_BYTES, CG_VECTOR_BYTES = 116, 96


def sphere_level_set(torch, n, device):
    ax = torch.arange(n + 1, device=device, dtype=torch.float64) / n
    cx, cy, cz, R = 0.47, 0.43, 0.41, 0.31
    d2 = (ax[:, None, None] - cz) ** 2 + (ax[None, :, None] - cy) ** 2 + (ax[None, None, :] - cx) ** 2
    return (torch.sqrt(d2) - R).reshape(-1).contiguous()


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def stats(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))


def run(n, k1, k2, repeats, solve):
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import fem, stokes
    device = torch.device("cuda", torch.cuda.current_device())
    mesh = cfx.Mesh.create_box(3, n)
    VU, VP = cfx.FunctionSpace(mesh, 1, bs=3), cfx.FunctionSpace(mesh, 1)
    system = stokes.build_blocks(VU, VP, cfx.cut(cfx.Function(VP, sphere_level_set(torch, n, device))))
    M, rows, _ = stokes.assemble(system)
    nu = VU.ndofs * VU.bs
    rows_u = rows[rows < nu].contiguous()
    indptr, _, _ = M.torch_views(device)
    lens = indptr[1:] - indptr[:-1]
    torch.manual_seed(0)
    b = torch.zeros(M.nrows, dtype=torch.float64, device=device)
    b[rows.long()] = torch.rand(rows.numel(), dtype=torch.float64, device=device) - 0.5
    info = fem.cg_info_buffer()

    def bytes_of(r, per_row):
        nr, nz = int(r.numel()), int(lens[r.long()].sum())
        return nr, nz, 12 * nz + 8 * (nr + 1) + 16 * nr + per_row * nr
    cases = {
        "minres_active": (rows, MINRES_VECTOR_BYTES, fem.minres_solve),
        "minres_velocity": (rows_u, MINRES_VECTOR_BYTES, fem.minres_solve),
        "cg_velocity": (rows_u, CG_VECTOR_BYTES, fem.cg_solve),
    }
    per = {name: [] for name in cases}
    for name, (r, _, fn) in cases.items():
        fn(M, b, rows=r, rtol=0.0, max_iter=2, check_every=0, info_out=info)     # warm-up
    for _ in range(repeats):
        for name, (r, _, fn) in cases.items():
            _, t1 = timed(torch, lambda: fn(M, b, rows=r, rtol=0.0, max_iter=k1, check_every=0, info_out=info))
            _, t2 = timed(torch, lambda: fn(M, b, rows=r, rtol=0.0, max_iter=k2, check_every=0, info_out=info))
            per[name].append((t2 - t1) / (k2 - k1))
    result = dict(n=n, rows=M.nrows, nnz=M.nnz, velocity_rows=nu, cases={})
    for name, (r, vec, _) in cases.items():
        nr, nz, nbytes = bytes_of(r, vec)
        s = stats(per[name])
        result["cases"][name] = dict(rows=nr, nnz=nz, mean_row=nz / nr, bytes=nbytes, iteration=s,
                                     fraction_of_stream=nbytes / (s["median_ms"] * 1e-3) / (STREAM_TBS * 1e12))
    c = result["cases"]
    predicted = c["cg_velocity"]["iteration"]["median_ms"] * c["minres_velocity"]["bytes"] / c["cg_velocity"]["bytes"]
    result["velocity_rows_prediction"] = dict(predicted_ms=predicted,
                                              measured_over_predicted=c["minres_velocity"]["iteration"]["median_ms"] / predicted)
    if solve:
        (_, i), t = timed(torch, lambda: fem.minres_solve(M, b, rows=rows, rtol=1e-8, max_iter=50000))
        result["solve_rtol_1e-8"] = dict(ms=t, iterations=i.iterations, reason=i.reason_name, residual=i.residual_norm / i.rhs_norm)
    return result


def table(r):
    lines = [f"n = {r['n']}: {r['rows']} rows ({r['velocity_rows']} velocity), nnz {r['nnz']}"]
    for name, m in r["cases"].items():
        it = m["iteration"]
        lines.append(f"  {name:16s} {m['rows']:>10d} rows, mean row {m['mean_row']:.1f}: {it['median_ms']:.4f} ms per iteration "
                     f"({it['min_ms']:.4f}-{it['max_ms']:.4f}), {m['bytes'] / 1e9:.4f} GB, {100 * m['fraction_of_stream']:.0f} % of "
                     f"{STREAM_TBS} TB/s")
    p = r["velocity_rows_prediction"]
    lines.append(f"  CG is timed over the active velocity rows alone (it breaks down on the indefinite matrix); MINRES on the same "
                 f"rows: predicted from CG by bytes {p['predicted_ms']:.4f} ms, measured / predicted {p['measured_over_predicted']:.2f}")
    if "solve_rtol_1e-8" in r:
        v = r["solve_rtol_1e-8"]
        lines.append(f"  solve to 1e-8 over the active rows: {v['iterations']} iterations, {v['ms']:.1f} ms ({v['reason']}, "
                     f"|r|/|b| {v['residual']:.1e})")
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, nargs="+", default=[128])
    p.add_argument("--iterations", type=int, nargs=2, default=[20, 120], help="the two iteration counts of a timed pair")
    p.add_argument("--repeats", type=int, default=5, help="batches per figure")
    p.add_argument("--no-solve", action="store_true", help="skip the whole solve to 1e-8")
    p.add_argument("--out", default=str(ROOT / "profiles"))
    args = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_minres: no GPU (nothing here is measured without one)")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    for n in args.n:
        r = run(n, args.iterations[0], args.iterations[1], args.repeats, not args.no_solve)
        (out / f"minres_n{n}.json").write_text(json.dumps(r, indent=1) + "\n")
        print(table(r), flush=True)


if __name__ == "__main__":
    main()
