"""Times a functional on the bench's workload (the n^3 sphere, default 512^3) on one GPU:

  (a) int_Omega u_h by the older route -- a SOURCE / F_COEFFICIENT linear form through fem.assemble_scalar: vector
      assembly, download of ndofs doubles, host sum;
  (b) the same by the rank-0 form M_FIELD (cfx_assemble_scalar, value left in HBM);
  (c) int_Omega (u_h - prod sin(pi x_i))^2 by M_L2_DIFF, which only the rank-0 route computes.

HIP events on the library stream (cfx_event_*), warm-up calls first, then `--repeat` timed calls each: median and
min / max.  (a) returns to the host, so its events bracket the download and the host sum as well.  The kernels' share
comes from cfx_profile_*; the achieved bandwidth is taken on the algorithmic bytes of the two functional kernels:
20 B per uncut cell (entity id + connectivity row; vertex and dof gathers are cache hits), 32 B per rule point + 28 B
per rule, 8 B per partial written and read.  Prints one JSON line.

    python tools/time_functional.py [--n 512] [--repeat 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HBM_PEAK_GBS = 8000.0  # MI355X spec (bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    import cutfemx_amd as cfx
    from bench import sphere_level_set
    from cutfemx_amd import _lib
    fem = cfx.fem
    dev = torch.device("cuda:0")
    n = args.n
    mesh = cfx.Mesh.create_box(3, n)
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, sphere_level_set(torch, n, dev)))
    inside = cfx.locate_entities_device(cd, "phi<0")
    rules = cfx.runtime_quadrature(cd, "phi<0", 4)
    # u_h: the interpolant of prod sin(pi x_i) plus a smooth perturbation, vertex id ix + (n+1)(iy + (n+1) iz)
    ax = torch.arange(n + 1, device=dev, dtype=torch.float64) / n
    s = torch.sin(torch.pi * ax)
    uh = (s[:, None, None] * s[None, :, None] * s[None, None, :] + 0.01 * ax[None, None, :] * ax[None, :, None]).reshape(-1).contiguous()
    uh = cfx.Function(V, uh)
    measure = dict(cells=inside, rules=rules)
    L = fem.form([fem.Integral(fem.SOURCE, params=(fem.F_COEFFICIENT, 1.0), qdegree=1, coefficient=uh, **measure)], V)
    Mf = fem.form([fem.Integral(fem.M_FIELD, params=(fem.F_COEFFICIENT, 1.0), qdegree=1, coefficient=uh, **measure)], V)
    Ml2 = fem.form([fem.Integral(fem.M_L2_DIFF, params=(fem.F_SINPROD, 1.0, 1.0), qdegree=4, coefficient=uh, **measure)], V)
    out = torch.zeros(1, device=dev, dtype=torch.float64)
    l = _lib.lib()

    def timed(fn):
        e0, e1 = C.c_void_p(), C.c_void_p()
        _lib.check(l.cfx_event_create(C.byref(e0)))
        _lib.check(l.cfx_event_create(C.byref(e1)))
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.repeat):
            _lib.check(l.cfx_event_record(e0))
            fn()
            _lib.check(l.cfx_event_record(e1))
            t = C.c_double()
            _lib.check(l.cfx_event_elapsed_ms(e0, e1, C.byref(t)))
            ms.append(t.value)
        _lib.check(l.cfx_event_destroy(e0))
        _lib.check(l.cfx_event_destroy(e1))
        return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    def profile(fn, reps=5):
        _lib.check(l.cfx_profile_enable(1))
        _lib.check(l.cfx_profile_reset())
        for _ in range(reps):
            fn()
        kernels = {}
        for i in range(l.cfx_profile_count()):
            name, ms, cnt = C.c_char_p(), C.c_double(), C.c_int64()
            _lib.check(l.cfx_profile_get(i, C.byref(name), C.byref(ms), C.byref(cnt)))
            if cnt.value:
                kernels[name.value.decode()] = dict(ms_per_call=round(ms.value / reps, 4), launches_per_call=cnt.value / reps)
        _lib.check(l.cfx_profile_enable(0))
        return kernels

    values = {}

    def run_a():
        values["a"] = fem.assemble_scalar(L)

    def run_b():
        fem.assemble_scalar(Mf, out=out)

    def run_c():
        fem.assemble_scalar(Ml2, out=out)

    res = {"n": n, "cells_inside": int(inside.size), "rules": int(rules.num_rules), "rule_points": int(rules.total_points)}
    res["a_source_vector_sum"] = timed(run_a)
    res["b_m_field"] = timed(run_b)
    values["b"] = float(out.cpu()[0])
    res["c_m_l2_diff"] = timed(run_c)
    values["c"] = float(out.cpu()[0])
    res["values"] = values
    res["b_kernels"] = profile(run_b)
    res["c_kernels"] = profile(run_c)
    partials = (inside.size + 255) // 256 + (rules.num_rules + 255) // 256
    alg_bytes = 20 * inside.size + 32 * rules.total_points + 28 * rules.num_rules + 16 * partials
    res["algorithmic_bytes"] = int(alg_bytes)
    for tag in ("b", "c"):
        k = res[f"{tag}_kernels"]
        ms = sum(k[name]["ms_per_call"] for name in ("functional_cells", "functional_reduce") if name in k)
        res[f"{tag}_kernel_ms"] = round(ms, 4)
        res[f"{tag}_achieved_GBs"] = round(alg_bytes / (ms * 1e-3) / 1e9, 1) if ms > 0 else None
        res[f"{tag}_hbm_fraction"] = round(alg_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms > 0 else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
