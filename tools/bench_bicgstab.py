#!/usr/bin/env python
"""Time BiCGStab in HBM (cutfemx_amd/csrc/cfx_solve.hip, cfx_bicgstab_solve) on the SUPG level-set matrix of supg.build_forms.

    python tools/bench_bicgstab.py --n 128 --out profiles

The SUPG matrix of the sphere level set of bench.py on Mesh.create_box(3, n) (speed = 1 + x_0, dt = 0.5 / n) is assembled
on the GPU (supg.assemble), and beside it the SPD matrix (grad u, grad v) + (u, v) over every cell of the same mesh -- the
Poisson matrix with the SAME sparsity, so both solvers multiply by the same number of entries.  Then, all rows iterated:

  ms per BiCGStab iteration  bicgstab_solve on the SUPG matrix, check_every = 0 and rtol = 0, for two iteration counts; the
                             difference removes the set-up launches
  ms per CG iteration        cg_solve on the Poisson matrix with max_iter fixed, check_every = 0 and rtol = 0, in the same
                             session, the two solvers taking turns batch by batch
  bytes per iteration        per product 12 nnz + 8 (rows + 1) + 16 rows (tools/bench_solve.py's count); BiCGStab makes two
                             products and moves 152 B per iterated row in its vector launches (bicg_half 40, bicg_update
                             64, bicg_direction 48), CG one product and 88 B (cg_update 56, cg_direction 32; no row list,
                             so no index is read); that figure over the time as a fraction of the 6.3 TB/s a streaming
                             kernel reaches on the MI355X
  prediction                 ms per CG iteration x (BiCGStab bytes / CG bytes): what BiCGStab should take if it follows
                             its byte count as CG does.  measured / predicted is the number to report
  the whole step             supg.advect to rtol = 1e-10: iterations, ms, reason

Every timed call must end with reason max_iter after exactly the iterations asked for (a breakdown would freeze the state
and the remaining launches would return at once): checked.  Batches end in a device synchronisation; median (min - max)
of `--repeats` pairs.  One JSON file per size (bicgstab_n<N>.json) and a table on stdout; nothing here runs without a GPU."""
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
BICGSTAB_VECTOR_BYTES, CG_VECTOR_BYTES = 152, 88


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
    import numpy as np
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import fem, supg
    device = torch.device("cuda", torch.cuda.current_device())
    mesh = cfx.Mesh.create_box(3, n)
    V = cfx.FunctionSpace(mesh, 1)
    phi = sphere_level_set(torch, n, device)
    speed = 1.0 + (torch.arange(n + 1, device=device, dtype=torch.float64) / n).repeat((n + 1) ** 2)   # x_0 runs fastest
    system = supg.build_forms(V, phi, speed, 0.5 / n)
    A, b = supg.assemble(system)
    cells = np.arange(mesh.num_cells, dtype=np.int32)
    P = fem.assemble_matrix(fem.form([fem.Integral(fem.STIFFNESS, cells=cells, qdegree=0),
                                      fem.Integral(fem.MASS, cells=cells, qdegree=2)], V))
    if (A.nrows, A.nnz) != (P.nrows, P.nnz):
        raise RuntimeError("the SUPG and the Poisson matrix differ in their sparsity")
    info = fem.cg_info_buffer()
    nbytes_product = 12 * A.nnz + 8 * (A.nrows + 1) + 16 * A.nrows
    cases = {
        "bicgstab_supg": (A, BICGSTAB_VECTOR_BYTES, 2, fem.bicgstab_solve),
        "cg_poisson": (P, CG_VECTOR_BYTES, 1, fem.cg_solve),
    }

    def call(fn, M, k):
        fn(M, b, rtol=0.0, max_iter=k, check_every=0, info_out=info)

    def ran(name, k):
        i = fem.read_cg_info(info)
        if i.reason != fem.CG_MAX_ITER or i.iterations != k:
            raise RuntimeError(f"{name}: stopped after {i.iterations} of {k} iterations ({i.reason_name}): the time is void")
    per = {name: [] for name in cases}
    for name, (M, _, _, fn) in cases.items():
        call(fn, M, 2)                                                             # warm-up
    for _ in range(repeats):
        for name, (M, _, _, fn) in cases.items():
            _, t1 = timed(torch, lambda: call(fn, M, k1))
            ran(name, k1)
            _, t2 = timed(torch, lambda: call(fn, M, k2))
            ran(name, k2)
            per[name].append((t2 - t1) / (k2 - k1))
    result = dict(n=n, rows=A.nrows, nnz=A.nnz, mean_row=A.nnz / A.nrows, cases={})
    for name, (M, vec, products, _) in cases.items():
        nbytes = products * nbytes_product + vec * A.nrows
        s = stats(per[name])
        result["cases"][name] = dict(bytes=nbytes, products=products, vector_bytes_per_row=vec, iteration=s,
                                     fraction_of_stream=nbytes / (s["median_ms"] * 1e-3) / (STREAM_TBS * 1e12))
    c = result["cases"]
    predicted = c["cg_poisson"]["iteration"]["median_ms"] * c["bicgstab_supg"]["bytes"] / c["cg_poisson"]["bytes"]
    result["prediction"] = dict(predicted_ms=predicted,
                                measured_over_predicted=c["bicgstab_supg"]["iteration"]["median_ms"] / predicted)
    if solve:
        (_, i), t = timed(torch, lambda: supg.advect(system, rtol=1e-10))
        result["advect_rtol_1e-10"] = dict(ms=t, iterations=i.iterations, reason=i.reason_name,
                                           residual=i.residual_norm / i.rhs_norm)
    return result


def table(r):
    lines = [f"n = {r['n']}: {r['rows']} rows, nnz {r['nnz']}, mean row {r['mean_row']:.1f}"]
    for name, m in r["cases"].items():
        it = m["iteration"]
        lines.append(f"  {name:14s} {it['median_ms']:.4f} ms per iteration ({it['min_ms']:.4f}-{it['max_ms']:.4f}), "
                     f"{m['bytes'] / 1e9:.4f} GB, {100 * m['fraction_of_stream']:.0f} % of {STREAM_TBS} TB/s")
    p = r["prediction"]
    lines.append(f"  BiCGStab predicted from CG by bytes {p['predicted_ms']:.4f} ms, measured / predicted "
                 f"{p['measured_over_predicted']:.2f}")
    if "advect_rtol_1e-10" in r:
        v = r["advect_rtol_1e-10"]
        lines.append(f"  supg.advect to 1e-10 (assembly and solve): {v['iterations']} iterations, {v['ms']:.1f} ms ({v['reason']}, "
                     f"|r|/|b| {v['residual']:.1e})")
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, nargs="+", default=[128])
    p.add_argument("--iterations", type=int, nargs=2, default=[20, 120], help="the two iteration counts of a timed pair")
    p.add_argument("--repeats", type=int, default=5, help="pairs per figure")
    p.add_argument("--no-solve", action="store_true", help="skip the whole step to 1e-10")
    p.add_argument("--out", default=str(ROOT / "profiles"))
    args = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_bicgstab: no GPU (nothing here is measured without one)")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    for n in args.n:
        r = run(n, args.iterations[0], args.iterations[1], args.repeats, not args.no_solve)
        (out / f"bicgstab_n{n}.json").write_text(json.dumps(r, indent=1) + "\n")
        print(table(r), flush=True)


if __name__ == "__main__":
    main()
