#!/usr/bin/env python
"""Time the solve in HBM (cutfemx_amd/csrc/cfx_solve.hip) on the sphere Poisson systems of bench.py.

    python tools/bench_solve.py --n 128 512 --out profiles

For every mesh size the P1 cut Poisson system is assembled and deactivated on the GPU, then, over ALL rows and over the
ACTIVE rows alone:

  ms per SpMV            fem.spmv, batches of calls between device synchronisations; median and range of the batches.
                         Twice: with L chosen by the library (a call then also counts the entries of the iterated rows
                         on the device -- with a row list, a pass over the list) and with the same L passed in (the
                         product alone, what a CG iteration contains)
  bytes per SpMV         12 nnz + 8 (rows + 1) + 16 rows  (values + indices, indptr, one read of x and one write of y per
                         row; nnz and rows those of the iterated rows), and that figure over the time as a fraction of
                         the 6.3 TB/s a streaming kernel reaches on the MI355X
  rocSPARSE yardstick    torch.sparse_csr_tensor @ x on the same matrix (all rows: it has no row list), its batches
                         alternating with ours in one loop so that both see the same machine
  ms per CG iteration    cg_solve with check_every = 0 and rtol = 0 for two iteration counts; the difference removes the
                         set-up launches
  iterations, total ms   cg_solve to rtol = 1e-8 for check_every in {1, 4, 16, 64}: the iteration count is the same for
                         all of them, the time shows what the host's looks and the launches after convergence cost

One JSON file per size (solve_n<N>.json) and a table on stdout.  Times are host clocks around work that ends in a
device synchronisation; nothing here runs without a GPU."""
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


def sphere_level_set(torch, n, device):
    ax = torch.arange(n + 1, device=device, dtype=torch.float64) / n
    cx, cy, cz, R = 0.47, 0.43, 0.41, 0.31
    d2 = (ax[:, None, None] - cz) ** 2 + (ax[None, :, None] - cy) ** 2 + (ax[None, None, :] - cx) ** 2
    return (torch.sqrt(d2) - R).reshape(-1).contiguous()


def batches(torch, fns, calls, repeats):
    """ms per call of every fn: `repeats` batches of `calls` calls each, the fns taking turns batch by batch."""
    out = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            out[i].append(1e3 * (time.perf_counter() - t0) / calls)
    return [dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for v in out]


def lanes_for(nnz, rows):
    """The library's choice of L (cfx_solve.hip: lanes_for)."""
    for lanes, per in ((1, 2), (4, 8), (8, 16), (16, 64)):
        if nnz <= per * rows:
            return lanes
    return 64


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def run(n, calls, repeats, sweep_all):
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import fem, poisson
    device = torch.device("cuda", torch.cuda.current_device())
    mesh = cfx.Mesh.create_box(3, n)
    V = cfx.FunctionSpace(mesh, 1)
    system = poisson.build_forms(V, cfx.cut(cfx.Function(V, sphere_level_set(torch, n, device))))
    A = fem.assemble_matrix(system.a)
    b = torch.zeros(V.ndofs, dtype=torch.float64, device=device)
    fem.assemble_vector(system.L, b)
    domain = fem.active_domain(system.a)
    fem.deactivate_outside(A, b, domain)
    active = fem.active_rows(domain)
    indptr, indices, values = A.torch_views(device)
    nnz_active = int((indptr[1:] - indptr[:-1])[active.long()].sum())
    x = torch.rand(A.nrows, dtype=torch.float64, device=device)
    y = torch.zeros_like(x)
    result = dict(n=n, rows=A.nrows, nnz=A.nnz, active_rows=int(active.numel()), active_nnz=nnz_active, modes={})

    # rocSPARSE through torch on the same arrays (int32 row pointers: nnz < 2^31)
    S = torch.sparse_csr_tensor(indptr.to(torch.int32), indices, values, size=(A.nrows, A.ncols))
    for mode, rows, nr, nz in (("all", None, A.nrows, A.nnz), ("active", active, int(active.numel()), nnz_active)):
        lanes = lanes_for(nz, nr)
        auto = lambda: fem.spmv(A, x, out=y, rows=rows)
        ours = lambda: fem.spmv(A, x, out=y, rows=rows, lanes_per_row=lanes)
        theirs = lambda: torch.mv(S, x)
        for _ in range(3):
            auto(); ours(); theirs()
        t_auto, t_ours, t_theirs = batches(torch, [auto, ours, theirs], calls, repeats)
        nbytes = 12 * nz + 8 * (nr + 1) + 16 * nr
        m = dict(rows=nr, nnz=nz, mean_row=nz / nr, lanes_per_row=lanes, spmv=t_ours, spmv_chosen=t_auto, spmv_bytes=nbytes,
                 spmv_fraction_of_stream=nbytes / (t_ours["median_ms"] * 1e-3) / (STREAM_TBS * 1e12))
        if rows is None:
            m["rocsparse"] = t_theirs
        # ms per iteration: two launch counts, no convergence (rtol = 0), no host look
        info = fem.cg_info_buffer()
        k1, k2 = 10, 40
        fem.cg_solve(A, b, rows=rows, rtol=0.0, max_iter=2, check_every=0, info_out=info)   # warm-up
        per = []
        for _ in range(repeats):
            _, t1 = timed(torch, lambda: fem.cg_solve(A, b, rows=rows, rtol=0.0, max_iter=k1, check_every=0, info_out=info))
            _, t2 = timed(torch, lambda: fem.cg_solve(A, b, rows=rows, rtol=0.0, max_iter=k2, check_every=0, info_out=info))
            per.append((t2 - t1) / (k2 - k1))
        m["iteration"] = dict(median_ms=statistics.median(per), min_ms=min(per), max_ms=max(per))
        # the whole solve to 1e-8, for several check_every
        if rows is not None or sweep_all:
            m["solve_rtol_1e-8"] = {}
            for ce in (1, 4, 16, 64):
                (_, i), t = timed(torch, lambda: fem.cg_solve(A, b, rows=rows, rtol=1e-8, check_every=ce, max_iter=20000))
                m["solve_rtol_1e-8"][str(ce)] = dict(ms=t, iterations=i.iterations, reason=i.reason_name,
                                                     residual=i.residual_norm / i.rhs_norm)
        result["modes"][mode] = m
    return result


def table(r):
    lines = [f"n = {r['n']}: {r['rows']} rows, nnz {r['nnz']}; {r['active_rows']} active rows, nnz {r['active_nnz']}"]
    for mode, m in r["modes"].items():
        s, it = m["spmv"], m["iteration"]
        line = (f"  {mode:6s} L {m['lanes_per_row']}: SpMV {s['median_ms']:.3f} ms ({s['min_ms']:.3f}-{s['max_ms']:.3f}; L chosen by the "
                f"library {m['spmv_chosen']['median_ms']:.3f}), {m['spmv_bytes'] / 1e9:.3f} GB, "
                f"{100 * m['spmv_fraction_of_stream']:.0f} % of {STREAM_TBS} TB/s; iteration {it['median_ms']:.3f} ms "
                f"({it['min_ms']:.3f}-{it['max_ms']:.3f})")
        if "rocsparse" in m:
            q = m["rocsparse"]
            line += f"; rocSPARSE {q['median_ms']:.3f} ms ({q['min_ms']:.3f}-{q['max_ms']:.3f})"
        lines.append(line)
        for ce, v in m.get("solve_rtol_1e-8", {}).items():
            lines.append(f"         check_every {ce:>2s}: {v['iterations']} iterations, {v['ms']:.1f} ms ({v['reason']}, "
                         f"|r|/|b| {v['residual']:.1e})")
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, nargs="+", default=[128, 512])
    p.add_argument("--calls", type=int, default=20, help="calls per timed batch")
    p.add_argument("--repeats", type=int, default=5, help="batches per figure")
    p.add_argument("--sweep-all-rows", action="store_true", help="also solve to 1e-8 over all rows (several times the work)")
    p.add_argument("--out", default=str(ROOT / "profiles"))
    args = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_solve: no GPU (nothing here is measured without one)")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    for n in args.n:
        r = run(n, args.calls, args.repeats, args.sweep_all_rows)
        (out / f"solve_n{n}.json").write_text(json.dumps(r, indent=1) + "\n")
        print(table(r), flush=True)


if __name__ == "__main__":
    main()
