#!/usr/bin/env python3
"""Benchmark of the cut-FEM hot path on MI355X.

One "step" = one full pass of the hot path on a synthetic level-set mesh whose
inputs (mesh connectivity, coordinates, level-set dof values) are already in
HBM:  classify -> locate -> sub-triangulate + runtime quadrature (phi<0, phi=0)
-> normals -> ghost-penalty facets -> forms -> CSR sparsity -> assemble_matrix
-> assemble_vector -> (N>1: RCCL row reduction) -> active domain + deactivation.
This is the per-time-step work of a moving-domain CutFEM solve
(python/demo/demo_moving_poisson.py:53-67); only the mesh-static incidence
tables (vertex->cells) are reused between steps.

Workload: BASELINE.json configs[2], the configuration its north-star target is
quoted on -- 3-D Poisson P1, sphere level set on the 512^3 background mesh
(805 M tets), Nitsche + ghost penalty, runtime quadrature order 4.  It fits one
MI355X (~60 GB), so N=1 runs it whole and N>1 strong-scales it over z-slabs.
`--n 128` runs configs[1]; the default N=1 run also reports it under
"config_128".

metric (BASELINE.json): assembled DOFs/s = active dofs / step time (whole job);
cut-quadrature points/s and per-phase times are reported beside it.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--mesh 512] [--order 4] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints the result line.  `--full` adds everything else the
benchmark measures (phase split, per-kernel HIP-event profile and rooflines, configs[1], [3], [4], the 32^3 and
implicit-structured lines, the moving-domain leg, the scaling projection, the CPU baselines) and writes the full record
to bench_detail.json.  `--dump-outputs DIR` writes what the last timed step computed (`dump_outputs`).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md (6.3 TB/s measured copy)

# ALGORITHMIC bytes per unit (explicit-connectivity variant)
B_CLASSIFY_PER_CELL = 18.3      # 16 B dofmap row + 8 B*V/C phi + 1 B domain
B_UNCUT_CELL = 60.0             # id 4 + geometry dofmap 16 + dofmap 16 + coords 4 + CSR write 20
B_QUAD_PER_POINT = 32.0         # (tdim+1)*8 written per emitted point (3-D)
B_QUAD_PER_CUT_CELL = 152.0     # dofmap 16 + coords 96 + phi 32 + offsets/parent 8
B_GHOST_FACET = 600.0           # SURVEY 8d's figure for a staged 8 x 8 facet tensor: row ids 16 + 2x(16+16) maps + 64 values x 8 B
# what the engine moves per ghost facet since round 2: the (c0, lf0, c1, lf1) row 16 B, the two cells' connectivity rows
# and vertices ~64 B, one 80 B rank-one record written by stage 1 (the kernel the profile calls assemble_facets) and read
# back by the interface-row gather
B_GHOST_FACET_RECORD = 80.0
B_GHOST_FACET_MOVED = 16.0 + 64.0 + 2 * B_GHOST_FACET_RECORD
# sparsity (not priced in SURVEY 8d): per marked cell its dofmap row (16 B) and its four
# incidence entries (16 B), per CSR entry 4 B written, per row 8 B of indptr
B_PATTERN_PER_CELL, B_PATTERN_PER_NNZ, B_PATTERN_PER_ROW = 32.0, 4.0, 8.0
B_SELECTOR_PER_CELL, B_SELECTOR_PER_HIT = 2.0, 4.0   # 1 B/cell x 2 passes + 4 B per located entity
B_NORMAL_PER_POINT = 24.0       # gdim doubles per interface point (a12)
B_VECTOR_PER_ROW_CELL = 16.0    # element-vector entry written once + read once per (row, cell) pair
B_DEACTIVATE_PER_ROW = 16.0     # diagonal write + rhs write per inactive row (a11)
FP64_VALU_PEAK_TFLOPS = 78.6    # MI355X FP64 vector = FP32 vector (157.3 TF, MI355X_MICROARCH.md) / 2; FP64 MFMA: the same rate
# flops of the source-term stage 1 per uncut cell: per point 3 x (5 offset + 2 x 5 series) + 3 products
# + 8 basis updates = 56, 11 points, + ~250 per cell (edges, determinant, 3 sincospi, 18 coefficients)
FLOP_SOURCE_PER_CELL = 11 * 56 + 250
# reference-equivalent quadrature size: Basix 0.11's default simplex scheme (Xiao-Gimbutas) has 11 points at degree 4
# on a tetrahedron and so has this engine's rule since round 3 (tools/gen_quadrature_tables.py: 11 positive interior
# points, symmetric about one vertex; rounds 1-2 used a 14-point rule); 6 = 6 on triangles
NQ_REF_PER_ENGINE_VOLUME, NQ_REF_PER_ENGINE_INTERFACE = 1.0, 1.0


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--mesh", "--n", dest="n", type=int, default=512,
                   help="background mesh n^3 cubes (x6 tets); use --mesh under torchrun (--n is ambiguous there)")
    p.add_argument("--order", type=int, default=4, help="runtime quadrature order (demo_poisson.py:139)")
    p.add_argument("--full", action="store_true",
                   help="also run what the headline figure does not need: phase split, per-kernel profile and rooflines, "
                        "the secondary configurations, the moving-domain leg, the scaling projection and the CPU baselines")
    p.add_argument("--dump-outputs", metavar="DIR",
                   help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (one GPU)")
    p.add_argument("--no-cpu", action="store_true", help="with --full: skip the cpu_baseline leg")
    p.add_argument("--cpu-n", type=int, default=256, help="mesh size of the bounded CPU sample (BASELINE.md 3: 256^3)")
    p.add_argument("--no-secondary", action="store_true",
                   help="with --full: skip the configs[1], [3], [4] and implicit-structured lines")
    p.add_argument("--cpu-worker", nargs=4, type=int, metavar=("N", "Z0", "Z1", "ORDER"),
                   help="internal: one process of the all-cores CPU baseline")
    args = p.parse_args()
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    return args


def sphere_level_set(torch, n, device):
    """phi = |x - c| - R sampled at the vertices, vertex id ix+(n+1)(iy+(n+1)iz)."""
    ax = torch.arange(n + 1, device=device, dtype=torch.float64) / n
    cx, cy, cz, R = 0.47, 0.43, 0.41, 0.31
    d2 = (ax[:, None, None] - cz) ** 2 + (ax[None, :, None] - cy) ** 2 + (ax[None, None, :] - cx) ** 2
    return (torch.sqrt(d2) - R).reshape(-1).contiguous()


class Timer:
    def __init__(self, torch):
        self.torch, self.t = torch, {}

    def run(self, name, fn):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        self.torch.cuda.synchronize()
        self.t[name] = self.t.get(name, 0.0) + (time.perf_counter() - t0)
        return out


def hot_path_step(cfx, poisson, V, phi_fn, values_buf, b_buf, order, timer=None, overlap=True):
    """One full pass on one GPU; returns counters.  `timer` splits the phases (extra syncs)."""
    run = (lambda name, fn: fn()) if timer is None else timer.run
    cd = run("cut", lambda: cfx.cut(phi_fn))
    system = run("rules+facets+forms", lambda: poisson.build_forms(V, cd, order=order))
    from cutfemx_amd import _lib
    import ctypes as C
    _lib.check(_lib.lib().cfx_device_memset(C.c_void_p(b_buf.data_ptr()), 0, C.c_size_t(8 * b_buf.numel())))   # b = 0
    if timer is None and overlap and os.environ.get("CFX_OVERLAP", "0") == "1":
        # opt-in (CFX_OVERLAP=1): L next to a on two HIP streams.  Measured at 512^3: 27.6 ms against 25.9 ms one after
        # the other -- every kernel of the step fills the chip on its own, a second lane only adds contention
        system.L.prepare()
        with cfx.fem.overlap() as lanes:
            lanes.side(lambda: cfx.fem.assemble_vector(system.L, b_buf))
            A = cfx.fem.create_matrix(system.a, values=values_buf)
            A.set_value(0.0)                                                                                      # A = 0
            cfx.fem.assemble_matrix(system.a, A=A)
    else:
        A = run("sparsity", lambda: cfx.fem.create_matrix(system.a, values=values_buf))
        A.set_value(0.0)                                                                                          # A = 0
        run("assemble_matrix", lambda: cfx.fem.assemble_matrix(system.a, A=A))
        run("assemble_vector", lambda: cfx.fem.assemble_vector(system.L, b_buf))
    dom = run("deactivate", lambda: cfx.fem.deactivate_outside(A, b_buf, cfx.fem.active_domain(system.a)))
    return StepResult(system, A, dom)


class StepResult:
    """What a step leaves behind; its counters are read from the engine on request -- after the step: inside a
    sync-free step (cutfemx_amd.run_step) the sizes are still in HBM and reading one would cost a round trip."""

    def __init__(self, system, A, dom):
        self.system, self.A, self.dom = system, A, dom

    def counts(self):
        system, A, dom = self.system, self.A, self.dom
        return dict(active_dofs=dom.num_active_dofs, nnz=A.nnz,
                    n_inside=system.inside_cells.size, n_cut=system.interface_rules.num_rules,
                    nq_volume=system.volume_rules.total_points, nq_interface=system.interface_rules.total_points,
                    n_vol_rules=system.volume_rules.num_rules,
                    n_ghost=0 if system.ghost_facets is None else system.ghost_facets.size)


DUMP_SAMPLE = 1 << 20      # entries kept of a dumped array longer than this: a fixed, seeded sample of them
DUMP_SEED = 1729
DUMP_COUNTS = ("active_dofs", "nnz", "n_inside", "n_cut", "nq_volume", "nq_interface", "n_vol_rules", "n_ghost")


def sample_positions(size, salt):
    """Sorted positions of the dumped sample of an array of `size` entries: all of them up to DUMP_SAMPLE, otherwise
    DUMP_SAMPLE positions drawn from the fixed seed (DUMP_SEED, salt) -- the same positions for the same length."""
    import numpy as np
    if size <= DUMP_SAMPLE:
        return np.arange(size, dtype=np.int64)
    return np.sort(np.random.default_rng([DUMP_SEED, salt]).integers(0, size, DUMP_SAMPLE, dtype=np.int64))


def dump_outputs(torch, res, b, device, out_dir):
    """What a caller of the timed path receives from its last step, as .npy files in `out_dir` (float64, the cell
    classification float32; under 64 MB in all): the CSR matrix (`A_values`, `A_indices`, `A_indptr`), the right-hand
    side `b`, the cell classification `domain` (-1 inside, 0 cut, +1 outside) and the `inactive_dofs` of the active
    domain, each sampled at `sample_positions`; `checksums` (sum, sum of |x|, sum of x^2 over the whole of A's values,
    then of b) and `counts` (DUMP_COUNTS) summarise the step."""
    import numpy as np
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    indptr, indices, values = res.A.torch_views(device)

    def take(name, t, salt, dtype=np.float64):
        pos = torch.from_numpy(sample_positions(int(t.numel()), salt)).to(t.device)
        np.save(out / f"{name}.npy", t[pos].cpu().numpy().astype(dtype))

    take("A_values", values, 1)
    take("A_indices", indices, 2)
    take("A_indptr", indptr, 3)
    take("b", b, 4)
    take("domain", torch.from_numpy(res.system.cut_data.domain()), 5, np.float32)
    take("inactive_dofs", torch.from_numpy(res.dom.inactive_dofs), 6)
    sums = [f(x).item() for x in (values, b) for f in (torch.sum, lambda v: v.abs().sum(), lambda v: (v * v).sum())]
    np.save(out / "checksums.npy", np.array(sums, dtype=np.float64))
    counts = res.counts()
    np.save(out / "counts.npy", np.array([counts[k] for k in DUMP_COUNTS], dtype=np.float64))


def cpu_baseline(n, order):
    """The CPU oracle (restatement of the reference loops, single thread) on the
    same workload at a bounded size; kind='port' because the reference itself
    cannot be built here.  The reference is serial per rank."""
    from helpers import level_set_values
    from oracle import pyoracle as O
    O.use_native_build()       # gcc -O3 -march=native on this host; results as the portable build
    om = O.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    t = {}

    def run(name, fn):
        t0 = time.perf_counter()
        out = fn()
        t[name] = time.perf_counter() - t0
        return out

    dom = run("cut", lambda: O.classify(om.conn, phi))
    inside = run("locate", lambda: O.locate_entities(dom, "phi<0"))
    vol = run("rules_volume", lambda: O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", order))
    itf = run("rules_interface", lambda: O.runtime_quadrature(om, om.conn, phi, dom, "phi=0", order))
    normals = run("normals", lambda: O.evaluate_normals(om, om.conn, phi, itf))
    ghost = run("ghost_facets", lambda: O.ghost_penalty_facets(om, dom, "phi<0"))
    V = O.Space(om.conn, om.nnodes, 1)
    a = [O.Integral(O.CELL, O.K_STIFFNESS, entities=inside, rules=vol, qdegree=0),
         O.Integral(O.CELL, O.K_NITSCHE, rules=itf, point_data=normals, params=(40.0,)),
         O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=ghost, params=(0.1,), qdegree=0)]
    L = [O.Integral(O.CELL, O.L_SOURCE, entities=inside, rules=vol, params=(O.F_POISSON_RHS, 1.0), qdegree=4),
         O.Integral(O.CELL, O.L_NITSCHE_RHS, rules=itf, point_data=normals, params=(40.0, O.F_SINPROD, 1.0))]
    indptr, indices = run("sparsity", lambda: O.create_sparsity(om, V, a))
    values = run("assemble_matrix", lambda: O.assemble_matrix(om, V, a, indptr, indices))
    b = run("assemble_vector", lambda: O.assemble_vector(om, V, L))

    def deact():
        act = O.active_cells(a, om.ncells)
        ina = O.inactive_dofs(V, act)
        O.deactivate(ina, indptr, indices, values, b)
        return ina
    ina = run("deactivate", deact)
    total = sum(t.values())
    active = om.nnodes - ina.size
    return dict(value=active / total, unit="DOF/s", cores=1, kind="port",
                sample=f"full hot path on the {n}^3 sphere workload ({6 * n ** 3} tets; oracle/cfx_oracle.c, "
                       f"gcc -O3 -march=native -ffp-contract=off, 1 thread), {total:.1f} s; the 512^3 case does not fit the "
                       "time budget of this leg: linear extrapolation in cells in `seconds_at_512_extrapolated`",
                seconds=total, seconds_at_512_extrapolated=total * (512.0 / n) ** 3, extrapolated=(n != 512),
                active_dofs=int(active),
                assemble_matrix_dofs_per_s=active / t["assemble_matrix"],
                cut_qp_per_s=(vol.weights.size + itf.weights.size)
                / (t["cut"] + t["rules_volume"] + t["rules_interface"]),
                phases_s={k: round(v, 4) for k, v in t.items()},
                host_cores_available=os.cpu_count())


def cpu_slab_worker(n, z0, z1, order):
    """One of `cores` CPU processes: the oracle hot path on the cell layers z0..z1-1 of the
    n^3 mesh (the reference's `mpirun -n cores` decomposition, without ghost layers)."""
    import numpy as np
    from helpers import level_set_values, oracle_poisson
    from oracle import pyoracle as O
    O.use_native_build()
    s2 = (n + 1) ** 2
    # layers z0..z1-1 of the n^3 Kuhn box (cutfemx_amd.mesh.box_mesh_arrays restricted to the slab)
    KUHN_TET = np.array([[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]])
    ax = np.arange(n + 1, dtype=np.float64) / n
    zz, yy, xx = np.meshgrid(np.arange(z0, z1 + 1, dtype=np.float64) / n, ax, ax, indexing="ij")
    x = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1)
    iz, iy, ix = np.meshgrid(np.arange(z1 - z0), np.arange(n), np.arange(n), indexing="ij")
    ix, iy, iz = ix.ravel(), iy.ravel(), iz.ravel()
    corner = np.stack([(ix + (i & 1)) + (n + 1) * ((iy + ((i >> 1) & 1)) + (n + 1) * (iz + ((i >> 2) & 1)))
                       for i in range(8)], axis=1)
    om = O.Mesh(3, x, np.ascontiguousarray(corner[:, KUHN_TET].reshape(-1, 4), dtype=np.int32))
    phi = level_set_values(om.x, 3)
    t0 = time.perf_counter()
    ref = oracle_poisson(O, om, phi, order=order)
    vals, b = ref["values"], ref["b"]
    O.deactivate(ref["inactive"], ref["indptr"], ref["indices"], vals, b)
    dt = time.perf_counter() - t0
    owned_hi = s2 * (z1 - z0 + (1 if z1 == n else 0))       # the lower rank owns a shared plane
    active = owned_hi - int(np.count_nonzero(ref["inactive"] < owned_hi))
    print(json.dumps(dict(seconds=dt, active=active)))


def cpu_baseline_all_cores(n, order):
    """The same CPU port run as one process per host core on z-slabs of the bounded sample:
    stand-in for the reference under `mpirun -n <cores>`.  Children are separate
    programs (no GPU use); throughput = active dofs / slowest process."""
    import subprocess

    from cutfemx_amd.dist import balanced_boundaries, sphere_layer_weights
    # a one-GPU box shares its host: its CPU share is 16 cores whatever os.cpu_count() says
    cores = max(1, min(os.cpu_count() or 1, 16, n // 4))
    bounds = balanced_boundaries(sphere_layer_weights(n), cores)   # the same weighted z-slabs as the GPU ranks
    procs = [subprocess.Popen([sys.executable, str(ROOT / "bench.py"), "--cpu-worker", str(n), str(bounds[i]),
                               str(bounds[i + 1]), str(order)], stdout=subprocess.PIPE, text=True,
                              env={**os.environ, "OMP_NUM_THREADS": "1"})
             for i in range(cores) if bounds[i + 1] > bounds[i]]
    outs = [json.loads(p.communicate()[0].strip().splitlines()[-1]) for p in procs]
    secs = max(o["seconds"] for o in outs)
    active = sum(o["active"] for o in outs)
    return dict(value=active / secs, unit="DOF/s", cores=len(procs), kind="port",
                sample=f"{n}^3 sphere workload split into {len(procs)} weighted z-slabs, one oracle process (gcc -O3 "
                       f"-march=native) per host core of this box's 16-core share (the box reports {os.cpu_count()} "
                       f"cores, a one-GPU job is allotted 16; no ghost layers), slowest process {secs:.1f} s",
                seconds=secs, active_dofs=active, host_cores_available=os.cpu_count())


def scale_fields(comm, world, per_rank_ms, exchange_ms):
    """What a SCALE-day line has to say about itself: which transport really moved the halo ('rccl': the library's own
    communicator; 'rccl-torch': the same links through the job's nccl process group when that communicator did not come
    up on every rank; an RCCL -> gloo fallback ends the job unless CFX_REHEARSE=1, cutfemx_amd.dist.decide_transport), on
    how many ranks the library's RCCL communicator came up, every rank's own step time (the slowest is the job's) and the
    exchange alone."""
    return dict(transport=comm.transport if comm is not None else "none", rccl_ranks=getattr(comm, "rccl_ranks", 0),
                world=world, per_rank_ms_per_step=[round(v, 4) for v in per_rank_ms],
                slowest_rank_ms_per_step=round(max(per_rank_ms), 4),
                imbalance=round(max(per_rank_ms) / (sum(per_rank_ms) / len(per_rank_ms)), 4),
                exchange_ms=round(exchange_ms, 4),
                exchange="level-set halo planes to / from the two slab neighbours, once per step (scatter_forward)",
                fallback_reason=getattr(comm, "fallback_reason", ""))


def kernel_profile(_lib, step, psteps):
    """Per-kernel HIP-event times (events on the launch stream) over psteps steps."""
    _lib.check(_lib.lib().cfx_profile_enable(1))
    _lib.check(_lib.lib().cfx_profile_reset())
    for _ in range(psteps):
        step()
    kernels = {}
    for i in range(_lib.lib().cfx_profile_count()):
        name, ms, cnt = C.c_char_p(), C.c_double(), C.c_int64()
        _lib.check(_lib.lib().cfx_profile_get(i, C.byref(name), C.byref(ms), C.byref(cnt)))
        if cnt.value:
            kernels[name.value.decode()] = dict(total_ms=ms.value / psteps, launches=cnt.value / psteps,
                                                avg_us=1e3 * ms.value / cnt.value)
    _lib.check(_lib.lib().cfx_profile_enable(0))
    return kernels


def measure(n, steps, warmup, order, world, rank, device, profile=True, dump_dir=None):
    """The timed steps of the n^3 workload.  `profile`: also the HIP-event split of the first step, the phase split,
    the per-kernel profile and the rooflines (extra steps after the timed region); `dump_dir`: write what the last
    timed step computed (`dump_outputs`, one GPU)."""
    import torch
    import torch.distributed as dist

    import cutfemx_amd as cfx
    from cutfemx_amd import _lib, poisson

    # ---- inputs resident in HBM before the timed region -----------------------
    if world == 1:
        mesh = cfx.Mesh.create_box(3, n)
        V = cfx.FunctionSpace(mesh, 1)
        phi_fn = cfx.Function(V, sphere_level_set(torch, n, device))
        # CSR value buffer: <= 15 (27 with ghost couplings) entries per active P1 row + 1 per inactive row
        nnz_cap = int(mesh.num_nodes) + 40 * int(0.2 * mesh.num_nodes + 100000)
        values_buf = torch.zeros(nnz_cap, device=device, dtype=torch.float64)
        b_buf = torch.zeros(mesh.num_nodes, device=device, dtype=torch.float64)

        # the timed step is a sync-free step of the moving-domain loop (cfx_step_begin / cfx_step_end): the sizes of its
        # lists stay in HBM, buffers are sized by the previous step's counts, one read-back ends it
        # (CFX_BENCH_STEP=0: every size read back where it is produced, as rounds 1-3 timed it)
        use_steps = os.environ.get("CFX_BENCH_STEP", "1") != "0"
        step_stats = {}

        def step(timer=None, overlap=True):
            if timer is not None or not use_steps:
                return hot_path_step(cfx, poisson, V, phi_fn, values_buf, b_buf, order, timer, overlap)
            return cfx.run_step(lambda: hot_path_step(cfx, poisson, V, phi_fn, values_buf, b_buf, order, None, overlap),
                                key=f"bench-{n}", info=step_stats)
    else:
        # z-slabs weighted by active cells, one rank per GPU, RCCL point-to-point row reduction
        from cutfemx_amd import dist as cdist
        mode = os.environ.get("CFX_DIST_MODE", "owner")   # "reduce": the reference's scatter_reverse flow
        part = (cdist.SlabPartition.create_owner(n, world, rank) if mode == "owner"
                else cdist.SlabPartition.create(n, world, rank))
        dp = cdist.DistributedPoisson(part, device, order=order, mode=mode)
        mesh = dp.mesh

        def step(timer=None, overlap=True):
            return dp.step() if timer is None else timer.run("step", dp.step)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # the first step also builds the mesh-static tables (dof -> cells incidence, row stencil, row tiles,
    # cell -> cell): timed on its own and reported as `setup_ms`, never part of `value`.  Its kernels are timed with
    # HIP events (the profile is on for this one step), so the rest of it -- the first allocation of the tables and
    # temporaries from the driver, code-object loading of kernels that run for the first time -- can be told apart
    mem0 = _lib.memory_stats(reset_peak=True)
    if profile:
        _lib.check(_lib.lib().cfx_profile_enable(1))
        _lib.check(_lib.lib().cfx_profile_reset())
    barrier()
    ts = time.perf_counter()
    info = step()
    barrier()
    first_step_ms = 1e3 * (time.perf_counter() - ts)
    first_kernels = {}
    if profile:
        for i in range(_lib.lib().cfx_profile_count()):
            name, ms, cnt = C.c_char_p(), C.c_double(), C.c_int64()
            _lib.check(_lib.lib().cfx_profile_get(i, C.byref(name), C.byref(ms), C.byref(cnt)))
            if cnt.value:
                first_kernels[name.value.decode()] = ms.value
        _lib.check(_lib.lib().cfx_profile_enable(0))
        _lib.check(_lib.lib().cfx_profile_reset())
    mem1 = _lib.memory_stats()
    # (the first step sized everything by read-backs; the next one takes its sizes from it and allocates the
    # capacity-sized buffers the timed steps then find in the block cache: it belongs to the setup, like the first)
    info = step()
    for _ in range(max(warmup - 1, 0)):
        info = step()
    barrier()
    syncs0 = _lib.sync_count()
    t0 = time.perf_counter()
    for _ in range(steps):
        info = step()
    barrier()
    elapsed = time.perf_counter() - t0
    read_backs = (_lib.sync_count() - syncs0) / steps
    last = None
    if world > 1:
        info = dp.counters(info)       # owned-share counts of the last step, outside the timed region
    else:
        last = info
        info = last.counts()
        if dump_dir is not None:
            dump_outputs(torch, last, b_buf, device, dump_dir)
    info = {k: v for k, v in info.items() if isinstance(v, (int, float))}
    scale_info = None
    if world > 1:
        cdev = device if dist.get_backend() == "nccl" else "cpu"
        # every rank's own time (the slowest one is the job's), and what the exchange alone costs
        mine = torch.tensor([elapsed / steps * 1e3], device=cdev, dtype=torch.float64)
        per_rank = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(per_rank, mine)
        xs = []
        for _ in range(3):
            barrier()
            tx = time.perf_counter()
            dp.exchange_only()
            torch.cuda.synchronize()
            xs.append(1e3 * (time.perf_counter() - tx))
        xm = torch.tensor([min(xs)], device=cdev, dtype=torch.float64)
        dist.all_reduce(xm, op=dist.ReduceOp.MAX)
        scale_info = scale_fields(dp.comm, world, [float(v.item()) for v in per_rank], float(xm.item()))
        t = torch.tensor([elapsed], device=cdev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        c = torch.tensor([float(info["active_dofs_owned"]), float(info["nq_volume"] + info["nq_interface"])],
                         device=cdev, dtype=torch.float64)
        dist.all_reduce(c, op=dist.ReduceOp.SUM)
        active_total, nq_total = float(c[0].item()), float(c[1].item())
    else:
        active_total = float(info["active_dofs"])
        nq_total = float(info["nq_volume"] + info["nq_interface"])
    out = dict(value=active_total / (elapsed / steps), ms_per_step=1e3 * elapsed / steps,
               active_dofs=int(active_total), counts={k: int(v) for k, v in info.items()})
    if scale_info is not None:
        out["multi_gpu"] = scale_info
    if world == 1:
        out["step_mode"] = dict(sync_free=use_steps, **step_stats, read_backs_per_step=read_backs,
                                note="sync_free: the timed step runs between cfx_step_begin / cfx_step_end -- list sizes stay "
                                     "in HBM (published), buffers are sized by the previous step's counts, one read-back ends "
                                     "the step; passes > 1 would mean a step was repeated because a count did not fit")
    static_bytes = (V if world == 1 else dp.V).static_table_bytes()
    setup_names = ("adj_", "stencil_", "cell_neighbours", "box_", "scan_reduce", "scan_write", "classify_summary")
    setup_kernel_ms = sum(v for k, v in first_kernels.items() if k.startswith(setup_names))
    first_kernel_ms = sum(first_kernels.values())
    mem2 = _lib.memory_stats()
    out["memory"] = dict(static_table_bytes=sum(static_bytes.values()), engine_bytes_in_use=mem2["in_use"],
                         engine_bytes_cached=mem2["cached"], engine_peak_bytes=mem2["peak"],
                         engine_bytes_before_first_step=mem0["in_use"] + mem0["cached"],
                         note="HBM held by the library's block cache (tables + temporaries + cached free blocks); the "
                              "caller's arrays (mesh, level set, CSR values, b) are not in it")
    out["setup"] = dict(setup_ms=first_step_ms - out["ms_per_step"], first_step_ms=first_step_ms,
                        steps_to_amortise=(first_step_ms - out["ms_per_step"]) / out["ms_per_step"],
                        split_ms=dict(setup_kernels=round(setup_kernel_ms, 2),
                                      other_kernels_of_the_first_step=round(first_kernel_ms - setup_kernel_ms, 2),
                                      allocation_module_load_host=round(first_step_ms - first_kernel_ms, 2))
                        if profile else None,
                        hbm_allocated_by_first_step_bytes=(mem1["in_use"] + mem1["cached"]) - (mem0["in_use"] + mem0["cached"]),
                        static_table_bytes=static_bytes, static_table_bytes_total=sum(static_bytes.values()),
                        note="mesh-static tables built by the first step and reused by every later one (moving-domain "
                             "loop: the level set changes, the mesh does not); not part of `value`")
    if not profile:
        return out

    # ---- phase split + per-kernel HIP-event profile: extra steps, same work -----
    psteps = max(2, min(steps, 5))
    timer = Timer(torch)
    for _ in range(psteps):
        step(timer)
    phases_ms = {k: round(1e3 * v / psteps, 4) for k, v in timer.t.items()}
    kernels = kernel_profile(_lib, lambda: step(overlap=False), psteps)   # one lane: every kernel alone on the GPU
    torch.cuda.synchronize()
    if "step_mode" in out:
        out["step_mode"]["launches_per_step"] = round(sum(v["launches"] for v in kernels.values()), 1)
        out["step_mode"]["launches_note"] = "kernel launches made by the library per step (its own launch wrapper: fills included)"
    # classification: the culled kernel (round 4) decides whole blocks of 1024 cells from the sign codes of their distinct
    # vertices and reads connectivity only in blocks the interface touches -- its algorithmic bytes are those of THAT
    # algorithm on this level set (the share of such blocks is taken from the domain array it produced), not the 18.3 B
    # per cell of the cell-by-cell loop, which `whole_step_roofline` keeps as SURVEY 8d prices the stage
    classify_bytes, classify_note = B_CLASSIFY_PER_CELL * mesh.num_cells, "cell by cell: 16 B dofmap row + level-set values + 1 B"
    if world == 1 and os.environ.get("CFX_CLASSIFY_CULL", "1") != "0":
        import numpy as np
        dom_h = last.system.cut_data.domain()
        nb = dom_h.size // 1024
        blk = dom_h[:nb * 1024].reshape(nb, 1024)
        uniform = (blk == blk[:, :1]).all(axis=1) & (blk[:, 0] != 0)
        mixed = 1.0 - float(uniform.mean()) if nb > 0 else 1.0
        # ... and inside those blocks quarter by quarter (256 cells) before any cell is looked at
        q = blk[~uniform].reshape(-1, 256)
        q_uniform = (q == q[:, :1]).all(axis=1) & (q[:, 0] != 0) if q.size else np.zeros(0, bool)
        mixed_cells = 256.0 * float((~q_uniform).sum())
        classify_bytes = (1.0 * mesh.num_cells + mesh.num_nodes + 256.0 * nb + 4 * 128.0 * float((~uniform).sum())
                          + 20.0 * mixed_cells)
        classify_note = (f"block culling: 1 B per cell written + 1 B per vertex code + 256 B of vertex runs per block of 1024 "
                         f"cells; {100.0 * mixed:.1f} % of the blocks have vertices on both sides and are decided by quarters "
                         f"(128 B of runs each), {100.0 * mixed_cells / max(mesh.num_cells, 1):.1f} % of the cells end in the "
                         "cell loop (20 B: connectivity row + codes)")
        del q
        del dom_h, blk
    alg_bytes = {
        "classify": classify_bytes,
        "assemble_rows": B_UNCUT_CELL * info["n_inside"],
        "assemble_rows_p1": B_UNCUT_CELL * info["n_inside"],
        "assemble_rows_plain": B_UNCUT_CELL * info["n_inside"],
        "pattern_rows": (B_PATTERN_PER_CELL * (info["n_inside"] + info["n_cut"]) + B_PATTERN_PER_NNZ * info["nnz"]
                         + B_PATTERN_PER_ROW * info.get("active_dofs", info.get("active_dofs_owned", 0))),
        # (both rule sets of a cut come out of ONE cut_emit launch since round 2; bytes per launch = total / launches)
        "cut_emit": (B_QUAD_PER_POINT * (info["nq_volume"] + info["nq_interface"])
                     + B_QUAD_PER_CUT_CELL * (info["n_vol_rules"] + info["n_cut"]))
                    / max(1.0, (kernels.get("cut_emit") or {}).get("launches", 1.0)),
        # stage 1 of the ghost penalty writes one 80 B record per facet (and reads the two cells: ~80 B)
        "assemble_facets": (B_GHOST_FACET_RECORD + 16.0 + 64.0) * info["n_ghost"],
    }
    alg_bytes["assemble_tiles_plain"] = alg_bytes["assemble_rows_plain"]   # the same rows by row tile
    if "assemble_rows_plain" in kernels or "assemble_tiles_plain" in kernels:   # the p1 kernel then only serves the interface rows
        alg_bytes.pop("assemble_rows_p1")
    if "plan_plain_masks" in kernels:         # the hashed kernel then only serves the interface rows
        alg_bytes.pop("pattern_rows")
        alg_bytes["plan_plain_masks"] = (B_PATTERN_PER_CELL * info["n_inside"] + B_PATTERN_PER_ROW
                                         * info.get("active_dofs", info.get("active_dofs_owned", 0)))
    roof = {}
    for name, ab in alg_bytes.items():
        if name in kernels and ab:
            ach = ab / (kernels[name]["avg_us"] * 1e-6) / 1e9
            roof[name] = dict(avg_us=round(kernels[name]["avg_us"], 2), algorithmic_bytes=ab,
                              achieved_GBs=round(ach, 1), frac=round(ach / HBM_PEAK_GBS, 4))
            if name == "classify":
                roof[name]["priced_as"] = classify_note
    # headline `roofline`: the dominant kernel of assemble_matrix, the phase BASELINE.json's metric is about (the
    # stage-2 kernel of the uncut cells); the other priced kernels -- classification, the longest HBM-priced kernel of
    # the step, included -- are in `roofline_by_kernel`, the longest kernel of all in `roofline_longest_kernel`
    priced = [k for k in kernels if alg_bytes.get(k)]
    matrix_kernels = [k for k in ("assemble_tiles_plain", "assemble_rows_plain", "assemble_rows_p1", "assemble_rows") if k in priced]
    dominant = (max(matrix_kernels, key=lambda k: kernels[k]["total_ms"]) if matrix_kernels
                else (max(priced, key=lambda k: kernels[k]["total_ms"]) if priced else None))
    roofline = None
    if dominant is not None:
        k = kernels[dominant]
        ab = alg_bytes.get(dominant)
        ach = None if ab is None else ab / (k["avg_us"] * 1e-6) / 1e9
        # HBM bytes per launch from the committed PMC passes (separate rocprofv3 --pmc runs of this
        # command, tools/profile_round.sh); only quoted for the mesh they were collected on
        traffic, tnote = None, "no PMC pass for this mesh in profiles/"
        tfiles = sorted((ROOT / "profiles").glob("r[0-9][0-9]_traffic.json"))
        if tfiles:
            t = json.loads(tfiles[-1].read_text())      # the latest round's passes
            e = t["kernels"].get(dominant)
            if t.get("mesh") == n and e and "fetch_bytes_raw" in e and "write_bytes" in e:
                # MI355X_MICROARCH.md, HBM: on gfx950 FETCH_SIZE reports half the bytes of a 16 B/lane coalesced
                # streaming read -- doubled for the kernels whose fetches are such streams (classify: one int4
                # dofmap row per lane); other access mixes are uncalibrated and quoted raw; WRITE_SIZE is exact
                streaming = dominant in ("classify",)   # (assemble_tiles_plain gathers: quoted raw)
                traffic = (2.0 if streaming else 1.0) * e["fetch_bytes_raw"] + e["write_bytes"]
                tnote = (f"FETCH_SIZE{' x 2 (gfx950 half-count of 16 B/lane streaming reads)' if streaming else ' (raw)'}"
                         f" + WRITE_SIZE per launch from {t['source']} (separate rocprofv3 --pmc passes, "
                         "tools/profile_round.sh); L2 hit rate "
                         + (f"{e['l2_hit_rate']:.2f}" if "l2_hit_rate" in e else "n/a"))
        roofline = dict(bound="hbm", kernel=dominant, achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=None if ach is None else ach / HBM_PEAK_GBS, traffic=traffic,
                        avg_launch_us=k["avg_us"], algorithmic_bytes_per_launch=ab,
                        note="achieved = SURVEY 8d bytes/unit x units of the launch / HIP-event duration on the "
                             f"launch stream, {psteps} profiled steps right after the timed region; traffic: " + tnote)
    # the kernel that takes longest, whatever bounds it (the headline `roofline` is the longest HBM-priced one)
    longest = max(kernels, key=lambda k: kernels[k]["total_ms"]) if kernels else None
    roofline_longest = None
    if longest == "vec_tensors_std":
        fl = FLOP_SOURCE_PER_CELL * info["n_inside"]
        ach = fl / (kernels[longest]["avg_us"] * 1e-6) / 1e12
        roofline_longest = dict(kernel=longest, bound="fp64-valu", achieved=ach, peak=FP64_VALU_PEAK_TFLOPS, unit="TFLOP/s",
                                frac=ach / FP64_VALU_PEAK_TFLOPS, avg_launch_us=kernels[longest]["avg_us"],
                                algorithmic_flops_per_launch=fl,
                                note="source term f v on the uncut cells: 11 points x (3 offsets + 3 short sine series) per "
                                     "tet; 4 scattered 8 B stores per cell on top (DESIGN.md 3)")
    elif longest is not None and longest in roof:
        roofline_longest = dict(kernel=longest, bound="hbm", achieved=roof[longest]["achieved_GBs"], peak=HBM_PEAK_GBS,
                                unit="GB/s", frac=roof[longest]["frac"], avg_launch_us=kernels[longest]["avg_us"])
    # whole step against the HBM roofline: SURVEY 8d's algorithmic bytes of every stage of one step / step time
    active = info.get("active_dofs", info.get("active_dofs_owned", 0))
    nrows = (n + 1) ** 3 if world == 1 else mesh.num_nodes
    step_bytes = dict(
        classify=B_CLASSIFY_PER_CELL * mesh.num_cells,
        selector_scans=B_SELECTOR_PER_CELL * mesh.num_cells + B_SELECTOR_PER_HIT * (info["n_inside"] + info["n_cut"]),
        quadrature=(B_QUAD_PER_POINT * (info["nq_volume"] + info["nq_interface"])
                    + B_QUAD_PER_CUT_CELL * (info["n_vol_rules"] + info["n_cut"])),
        normals=B_NORMAL_PER_POINT * info["nq_interface"],
        ghost_facets=B_GHOST_FACET_MOVED * info["n_ghost"],
        sparsity=(B_PATTERN_PER_CELL * (info["n_inside"] + info["n_cut"]) + B_PATTERN_PER_NNZ * info["nnz"]
                  + B_PATTERN_PER_ROW * nrows),
        matrix_uncut_cells=B_UNCUT_CELL * info["n_inside"],
        matrix_cut_cells=(B_UNCUT_CELL * (info["n_vol_rules"] + info["n_cut"])
                          + B_QUAD_PER_POINT * (info["nq_volume"] + info["nq_interface"])
                          + B_NORMAL_PER_POINT * info["nq_interface"]),
        matrix_zero=8.0 * (nrows - active),    # set_value(0) is fused: only the inactive rows' diagonal entries are zeroed
        vector=B_VECTOR_PER_ROW_CELL * 4 * info["n_inside"] + 8.0 * nrows,
        deactivate=B_DEACTIVATE_PER_ROW * (nrows - active))
    total_bytes = float(sum(step_bytes.values()))
    # ... and on the bytes of the algorithms the step actually runs: the culled classification does not stream the
    # connectivity (its own price, `classify_bytes` above), everything else is priced as it is moved already
    moved_bytes = total_bytes - step_bytes["classify"] + float(classify_bytes)
    step_s = out["ms_per_step"] * 1e-3
    whole_step = dict(algorithmic_bytes=total_bytes, achieved=total_bytes / step_s / 1e9,
                      peak=HBM_PEAK_GBS, unit="GB/s", frac=total_bytes / step_s / 1e9 / HBM_PEAK_GBS,
                      frac_survey_bytes=total_bytes / step_s / 1e9 / HBM_PEAK_GBS,
                      frac_moved_bytes=moved_bytes / step_s / 1e9 / HBM_PEAK_GBS,
                      moved_bytes=moved_bytes,
                      fractions_are="frac_survey_bytes: SURVEY 8d's bytes per unit for every stage (18.3 B per cell for the "
                                    "classification, which the block-culled kernel does not move); frac_moved_bytes: the same "
                                    "sum with the classification priced as the culled algorithm moves it",
                      bytes_by_stage={k: float(v) for k, v in step_bytes.items()},
                      note="SURVEY 8d bytes per unit x units of this step (explicit connectivity), summed over the "
                           "stages, / measured step time; ghost facets and the zero fill priced as the engine moves them "
                           "(one 80 B record per facet written + read, inactive rows only) -- SURVEY's 600 B facet tensor "
                           "and an 8 B x nnz fill would add " + f"{(B_GHOST_FACET - B_GHOST_FACET_MOVED) * info['n_ghost'] + 8.0 * (info['nnz'] - (nrows - active)):.3g} B")
    nq_ref = NQ_REF_PER_ENGINE_VOLUME * info["nq_volume"] + NQ_REF_PER_ENGINE_INTERFACE * info["nq_interface"]
    out.update(phases_ms=phases_ms, roofline_longest_kernel=roofline_longest, whole_step_roofline=whole_step,
               cut_quadrature_points_reference_equivalent=dict(
                   points=nq_ref,
                   points_per_s=(nq_ref * (nq_total / max(info["nq_volume"] + info["nq_interface"], 1))
                                 / (1e-3 * (phases_ms["cut"] + phases_ms["rules+facets+forms"]))
                                 if "cut" in phases_ms else None),
                   note="the engine's degree-4 tetrahedron rule has 11 points, as Basix's (the reference's): the point "
                        "counts are the reference's (the points themselves are not: parity unpinned below integral level)"),
               cut_quadrature_points_per_s=(nq_total / (1e-3 * (phases_ms["cut"] + phases_ms["rules+facets+forms"]))
                                            if "cut" in phases_ms else None),
               assemble_matrix_dofs_per_s=(active_total / (1e-3 * phases_ms["assemble_matrix"])
                                           if "assemble_matrix" in phases_ms else None),
               kernels={k: {kk: round(vv, 3) for kk, vv in v.items()}
                        for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["total_ms"])},
               roofline=roofline, roofline_by_kernel=roof)
    return out


def _timed_steps(torch, step, steps=3, warmup=1):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        info = step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, info


def _kernel_times(step):
    import cutfemx_amd
    from cutfemx_amd import _lib
    k = kernel_profile(_lib, step, 1)
    return {n: round(v["total_ms"], 2) for n, v in sorted(k.items(), key=lambda kv: -kv[1]["total_ms"])[:10]}


def phase_roofline(tag, phase, ms, alg_bytes, what):
    """Roofline entry of one phase of a secondary configuration: algorithmic bytes / measured phase time against the
    HBM peak, with the phase's counter traffic from the committed PMC passes (tools/profile_cfg45.sh ->
    tools/pmc_phase_traffic.py -> profiles/rNN_<tag>_traffic.json: the latest round's file is quoted and named) beside it."""
    traffic, tnote, kern = None, "no PMC pass for this workload in profiles/", None
    files = sorted((ROOT / "profiles").glob(f"r[0-9][0-9]_{tag}_traffic.json"))
    if files:
        f = files[-1]
        t = json.loads(f.read_text())
        traffic = t["phase_traffic_bytes"]
        kern = {k.split("(")[0][:60]: {kk: vv for kk, vv in v.items() if kk in ("wait_any_share", "l2_hit_rate")}
                for k, v in t["kernels"].items()}
        tnote = (f"FETCH_SIZE (raw) + WRITE_SIZE of the phase's kernels per step from {t['source']} via profiles/{f.name} "
                 "(separate rocprofv3 --pmc passes of the same program, tools/profile_cfg45.sh)")
    ach = alg_bytes / (ms * 1e-3) / 1e9
    return dict(bound="hbm", kernel=phase, achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach / HBM_PEAK_GBS,
                traffic=traffic, algorithmic_bytes=alg_bytes, phase_ms=ms, algorithmic_bytes_are=what,
                counters_by_kernel=kern, note=tnote)


def engine_memory(V, _lib):
    sb = V.static_table_bytes()
    m = _lib.memory_stats()
    return dict(static_table_bytes=sb, static_table_bytes_total=sum(sb.values()), engine_peak_bytes=m["peak"],
                engine_bytes_in_use=m["in_use"], engine_bytes_cached=m["cached"])


def secondary_p2_gyroid(torch, device, n=256):
    """BASELINE configs[3]: 3-D Poisson, gyroid level set (k = 4) on the 256^3 mesh, P2 solution space over the P1
    level set, Nitsche + ghost penalty, order 4.  Step = rules + forms + sparsity + assemble_matrix +
    assemble_vector + deactivation with the cut (classification) included."""
    import math

    import cutfemx_amd as cfx
    from cutfemx_amd import fem, poisson
    mesh = cfx.Mesh.create_box(3, n)
    Vphi = cfx.FunctionSpace(mesh, 1)
    ax = torch.arange(n + 1, device=device, dtype=torch.float64) / n
    Z, Y, X = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    k = 2.0 * math.pi * 4.0
    def gyroid(shift=0.0):
        Xs = X + shift
        return (torch.sin(k * Xs) * torch.cos(k * Y) + torch.sin(k * Y) * torch.cos(k * Z) + torch.sin(k * Z) * torch.cos(k * Xs)
                + 0.0137).reshape(-1).contiguous()
    phi_values = gyroid()
    phi = cfx.Function(Vphi, phi_values)
    dm, nd = cfx.box_lagrange2_dofmap(mesh, n, device)
    V = cfx.FunctionSpace(mesh, 2, dofmap=dm, ndofs=nd)
    b = torch.zeros(nd, device=device, dtype=torch.float64)
    phases = {}

    def step():
        t = time.perf_counter
        torch.cuda.synchronize(); t0 = t()
        cd = cfx.cut(phi)
        sysm = poisson.build_forms(V, cd, order=4)
        torch.cuda.synchronize(); t1 = t()
        A = fem.create_matrix(sysm.a)
        torch.cuda.synchronize(); t2 = t()
        fem.assemble_matrix(sysm.a, A=A)
        torch.cuda.synchronize(); t3 = t()
        b.zero_()
        fem.assemble_vector(sysm.L, b)
        dom = fem.deactivate_outside(A, b, fem.active_domain(sysm.a))
        torch.cuda.synchronize(); t4 = t()
        phases.update(cut_rules_forms=1e3 * (t1 - t0), sparsity=1e3 * (t2 - t1), assemble_matrix=1e3 * (t3 - t2),
                      assemble_vector_deactivate=1e3 * (t4 - t3))
        return dict(active_dofs=dom.num_active_dofs, nnz=A.nnz, n_inside=sysm.inside_cells.size,
                    n_cut=sysm.interface_rules.num_rules, nq_volume=sysm.volume_rules.total_points,
                    nq_interface=sysm.interface_rules.total_points,
                    n_ghost=0 if sysm.ghost_facets is None else sysm.ghost_facets.size)
    from cutfemx_amd import _lib
    _lib.memory_stats(reset_peak=True)
    # (the step re-cuts ONE level set: every pattern row would be "unchanged since the last step" -- the row reuse of
    # moving-domain loops is switched off for this line, which stays a full rebuild as in rounds 1-3, and measured on a
    # gyroid that really moves below)
    os.environ["CFX_PATTERN_REUSE"] = "0"
    try:
        ms, info = _timed_steps(torch, step, steps=2, warmup=1)
        kernels_ms = _kernel_times(step)
        # the same calls as ONE step of the moving-domain loop (cutfemx_amd.run_step): sizes published where the engine
        # defers them (the plan, the rules, nnz), the rest read back on demand -- a hashed space is not sync-free yet
        def body():
            cd = cfx.cut(phi)
            sysm = poisson.build_forms(V, cd, order=4)
            A = fem.create_matrix(sysm.a)
            fem.assemble_matrix(sysm.a, A=A)
            b.zero_()
            fem.assemble_vector(sysm.L, b)
            return fem.deactivate_outside(A, b, fem.active_domain(sysm.a))
        in_step = {}
        for kk in range(4):
            torch.cuda.synchronize(); s0 = _lib.sync_count(); t0 = time.perf_counter()
            sinfo = {}
            out_step = cfx.run_step(body, key=f"bench-p2-{n}", info=sinfo)
            torch.cuda.synchronize()
            if kk >= 2:
                in_step.setdefault("ms", []).append(1e3 * (time.perf_counter() - t0))
                in_step["read_backs"] = _lib.sync_count() - s0
                in_step["passes"] = sinfo.get("passes")
            del out_step
        in_step["ms_per_step"] = round(sum(in_step.pop("ms")) / 2, 2)
    finally:
        os.environ.pop("CFX_PATTERN_REUSE", None)

    def moving(reuse, nsteps=4, shift_h=0.3):
        """create_matrix of the MOVING gyroid (shifted by shift_h cells along x per step), with and without row reuse"""
        os.environ["CFX_PATTERN_REUSE"] = "1" if reuse else "0"
        try:
            times, stats = [], []
            for kk in range(-1, nsteps):      # one untimed step: the cache then holds the pattern one shift back
                phi_values.copy_(gyroid(shift_h * kk / n))
                torch.cuda.synchronize()
                cd = cfx.cut(phi)
                sysm = poisson.build_forms(V, cd, order=4)
                torch.cuda.synchronize(); t1 = time.perf_counter()
                A = fem.create_matrix(sysm.a)
                torch.cuda.synchronize(); t2 = time.perf_counter()
                if kk >= 0:
                    times.append(1e3 * (t2 - t1))
                    stats.append(A.reuse_stats)
                del A, sysm, cd
            return dict(create_matrix_ms=round(sum(times) / len(times), 2),
                        create_matrix_median_ms=round(sorted(times)[len(times) // 2], 2),
                        each_ms=[round(t, 2) for t in times],
                        hashed_rows=stats[-1][0], reused_rows=stats[-1][1],
                        reused_share=round(stats[-1][1] / max(stats[-1][0], 1), 4))
        finally:
            os.environ.pop("CFX_PATTERN_REUSE", None)
    moving_leg = {"what": f"gyroid shifted by 0.3 h along x per step: create_matrix with the rows around unchanged cells "
                          "copied from the previous pattern of the space (cfx_pattern_reuse_stats) against a full rebuild",
                  "incremental": moving(True), "full_rebuild": moving(False)}
    phi_values.copy_(gyroid())
    # algorithmic bytes (SURVEY 8d style): assemble_matrix = CSR values written once + per uncut cell its connectivity
    # row, its share of the vertex coordinates and its degree-2 dofmap row + the rule slices of the cut cells (points,
    # weights, normals) + one record per ghost facet; sparsity = indices + indptr written + the same cell streams
    cell_b = 16.0 + 4.0 + 40.0
    mat_b = (8.0 * info["nnz"] + cell_b * (info["n_inside"] + 2 * info["n_cut"])
             + 32.0 * info["nq_volume"] + 56.0 * info["nq_interface"] + 448.0 * info["n_ghost"])
    pat_b = 4.0 * info["nnz"] + 8.0 * nd + (16.0 + 40.0) * (info["n_inside"] + info["n_cut"])
    return dict(workload=f"configs[3]: 3D Poisson, gyroid level set on the {n}^3 mesh ({6 * n ** 3} tets), P2 space "
                         f"({nd} dofs) over the P1 level set, Nitsche + ghost penalty, order 4; one step = cut + rules + "
                         "sparsity + assemble_matrix + assemble_vector + deactivation",
                value=info["active_dofs"] / (1e-3 * ms), unit="DOF/s", ms_per_step=ms, counts=info,
                phases_ms={k2: round(v, 2) for k2, v in phases.items()}, kernels_ms=kernels_ms,
                as_one_step=dict(in_step, note="the same calls inside cutfemx_amd.run_step, no synchronisation between the "
                                               "phases: `ms_per_step` above is the plain sequence timed phase by phase"),
                moving_domain=moving_leg,
                roofline=phase_roofline("cfg4", "assemble_matrix (phase)", phases["assemble_matrix"], mat_b,
                                        "8 B x nnz values + 60 B per uncut / cut cell + rule slices + 448 B per ghost facet"),
                roofline_sparsity=phase_roofline("cfg4_sparsity", "create_matrix (phase)", phases["sparsity"], pat_b,
                                                 "4 B x nnz indices + 8 B per row + 56 B per marked cell"),
                memory=engine_memory(V, _lib))


def secondary_elasticity_share(torch, device, n=256, z0=89, nz=32):
    """BASELINE configs[4] is an 8-GPU configuration: this is ONE rank's share of it (a 256 x 256 x 32 slab of the
    256^3 mesh through the sphere), P2 vector space, sigma(u):eps(v) over [solid cells, rules] + ghost penalty
    (python/demo/demo_elasticity.py:214-235).  Step = cut + rules + sparsity + assemble_matrix."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    mesh = cfx.Mesh.create_slab(n, z0, nz)
    Vphi = cfx.FunctionSpace(mesh, 1)
    ax = torch.arange(n + 1, device=device, dtype=torch.float64) / n
    az = torch.arange(z0, z0 + nz + 1, device=device, dtype=torch.float64) / n
    d2 = (az[:, None, None] - 0.41) ** 2 + (ax[None, :, None] - 0.43) ** 2 + (ax[None, None, :] - 0.47) ** 2
    phi = cfx.Function(Vphi, (torch.sqrt(d2) - 0.31).reshape(-1).contiguous())
    dm, nd = cfx.box_lagrange2_dofmap(mesh, n, device)
    V = cfx.FunctionSpace(mesh, 2, dofmap=dm, ndofs=nd, bs=3)
    E, nu = 1.0e3, 0.3
    mu, lmbda = E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    phases = {}

    def step():
        t = time.perf_counter
        torch.cuda.synchronize(); t0 = t()
        cd = cfx.cut(phi)
        inside = cfx.locate_entities_device(cd, "phi<0")
        vol = cfx.runtime_quadrature(cd, "phi<0", 2)
        ghost = cfx.ghost_penalty_facets(cd, "phi<0")
        a = fem.form([fem.Integral(fem.ELASTICITY, cells=inside, rules=vol, params=(E, nu), qdegree=2),
                      fem.Integral(fem.GHOST_GRADJUMP, facets=ghost, params=(0.05 * (2.0 * mu + lmbda),), qdegree=2)], V)
        torch.cuda.synchronize(); t1 = t()
        A = fem.create_matrix(a)
        torch.cuda.synchronize(); t2 = t()
        fem.assemble_matrix(a, A=A)
        torch.cuda.synchronize(); t3 = t()
        phases.update(cut_rules_forms=1e3 * (t1 - t0), sparsity=1e3 * (t2 - t1), assemble_matrix=1e3 * (t3 - t2))
        dom = fem.active_domain(a)
        return dict(active_dofs=dom.num_active_dofs, nnz=A.nnz, n_inside=inside.size, n_ghost=ghost.size,
                    n_cut=vol.num_rules, nq_volume=vol.total_points)
    from cutfemx_amd import _lib
    _lib.memory_stats(reset_peak=True)
    os.environ["CFX_PATTERN_REUSE"] = "0"      # a full rebuild, as in rounds 1-3 (the step re-cuts one level set)
    try:
        ms, info = _timed_steps(torch, step, steps=2, warmup=1)
        kernels_ms = _kernel_times(step)
    finally:
        os.environ.pop("CFX_PATTERN_REUSE", None)
    # assemble_matrix: the CSR values written once (8 B x nnz: 11.5 GB here) + per cell its connectivity row, vertex
    # share and degree-2 dofmap row + the cut cells' rule slices + the ghost-facet records.  Flops of the phase: the
    # closed-form block rows, ~50 flop per 3 x 3 block, 100 blocks per (cell, row dof) pair-set: 3 x 10^4 per cell
    mat_b = 8.0 * info["nnz"] + 60.0 * (info["n_inside"] + info["n_cut"]) + 32.0 * info["nq_volume"] + 448.0 * info["n_ghost"]
    pat_b = 4.0 * info["nnz"] + 8.0 * 3 * nd + 56.0 * (info["n_inside"] + info["n_cut"])
    return dict(workload=f"configs[4], one of eight ranks' share: layers {z0}..{z0 + nz - 1} of the {n}^3 mesh, sphere level "
                         f"set, P2 vector space (3 x {nd} dofs), elasticity + ghost penalty; one step = cut + rules + sparsity "
                         "+ assemble_matrix",
                value=info["active_dofs"] / (1e-3 * ms), unit="DOF/s", ms_per_step=ms, counts=info,
                phases_ms={k2: round(v, 2) for k2, v in phases.items()}, kernels_ms=kernels_ms,
                roofline=phase_roofline("cfg5", "assemble_matrix (phase)", phases["assemble_matrix"], mat_b,
                                        "8 B x nnz values + 60 B per cell + rule slices + 448 B per ghost facet"),
                roofline_sparsity=phase_roofline("cfg5_sparsity", "create_matrix (phase)", phases["sparsity"], pat_b,
                                                 "4 B x nnz indices + 8 B per row + 56 B per marked cell"),
                memory=engine_memory(V, _lib))


def launcher_command(args, port=None):
    """The command line of the N-rank job `python3 bench.py --gpus N` starts when nobody launched the ranks for it
    (WORLD_SIZE unset): one process per GPU under torch.distributed.run, rendezvous on 127.0.0.1."""
    if port is None:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(ROOT / "bench.py"),
           "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--mesh", str(args.n), "--order", str(args.order), "--cpu-n", str(args.cpu_n)]
    if args.no_cpu:
        cmd.append("--no-cpu")
    if args.no_secondary:
        cmd.append("--no-secondary")
    if getattr(args, "full", False):
        cmd.append("--full")
    return cmd


def launch_ranks(args):
    """`python3 bench.py --gpus N` with WORLD_SIZE unset: start the N ranks as a CHILD process (never exec: nothing
    in this process has touched HIP or imported torch yet, and it stays that way), relay the child's output -- rank 0
    prints the one JSON line -- and return its exit code."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    return run_child(launcher_command(args), env, float(os.environ.get("CFX_BENCH_TIMEOUT", "3000")))


def run_child(cmd, env, timeout_s):
    """Start `cmd` as a child in its own process group, relay its stdout line by line, return its exit code.  A rank
    that dies takes the job down through torch.distributed.run (non-zero exit); a job that hangs -- a rank stuck in a
    collective whose peer is gone -- is killed as a group after `timeout_s` and reported as 124."""
    import signal
    import subprocess
    import threading
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)

    def relay():
        for line in proc.stdout:
            sys.stdout.write(line)
            sys.stdout.flush()
    t = threading.Thread(target=relay, daemon=True)
    t.start()
    try:
        rc = proc.wait(timeout=timeout_s)
    except subprocess.TimeoutExpired:
        sys.stderr.write(f"bench.py: the rank job did not finish within {timeout_s:.0f} s: killing its process group\n")
        for sig in (signal.SIGTERM, signal.SIGKILL):
            try:
                os.killpg(proc.pid, sig)      # the exact group this call started (start_new_session), nothing else
            except ProcessLookupError:
                break
            try:
                proc.wait(timeout=10)
                break
            except subprocess.TimeoutExpired:
                continue
        rc = 124
    t.join(timeout=5)
    return rc


def moving_domain_leg(torch, device, n, order, nsteps=8, shift_h=0.3):
    """The loop the step stands for, with the interface really MOVING (python/demo/demo_moving_poisson.py:53-90): one
    CutData, the sphere's centre advanced by `shift_h` cells per step, cut.update() + rules + forms + create_matrix +
    assemble + deactivation every step.  Timed twice over the same positions: as sync-free steps (cutfemx_amd.run_step:
    sizes from the previous step, one read-back per step) and with every size read back where it is produced.  The
    headline `value` re-cuts ONE level set; here the counts of every step differ from the last step's."""
    import cutfemx_amd as cfx
    from cutfemx_amd import _lib, poisson
    mesh = cfx.Mesh.create_box(3, n)
    V = cfx.FunctionSpace(mesh, 1)
    ax = torch.arange(n + 1, device=device, dtype=torch.float64) / n
    phi = torch.empty((n + 1) ** 3, device=device, dtype=torch.float64)
    f = cfx.Function(V, phi)
    values = torch.zeros(int(mesh.num_nodes) + 40 * int(0.2 * mesh.num_nodes + 100000), device=device, dtype=torch.float64)
    b = torch.zeros(mesh.num_nodes, device=device, dtype=torch.float64)
    state = {"cd": None}

    def place(k):
        cx, cy, cz, R = 0.40 + shift_h * k / n, 0.43, 0.41, 0.31
        d2 = (ax[:, None, None] - cz) ** 2 + (ax[None, :, None] - cy) ** 2 + (ax[None, None, :] - cx) ** 2
        phi.copy_((torch.sqrt(d2) - R).reshape(-1))     # in place: the engine aliases this array

    def body():
        if state["cd"] is None:
            state["cd"] = cfx.cut(f)
        else:
            cfx.update(state["cd"])
        system = poisson.build_forms(V, state["cd"], order=order)
        _lib.check(_lib.lib().cfx_device_memset(C.c_void_p(b.data_ptr()), 0, C.c_size_t(8 * b.numel())))
        A = cfx.fem.create_matrix(system.a, values=values)
        A.set_value(0.0)
        cfx.fem.assemble_matrix(system.a, A=A)
        cfx.fem.assemble_vector(system.L, b)
        dom = cfx.fem.deactivate_outside(A, b, cfx.fem.active_domain(system.a))
        return StepResult(system, A, dom)

    def run(sync_free, key):
        cfx.forget_step_history(key)
        times, passes, syncs, nnz = [], [], [], []
        for k in range(-2, nsteps):          # two untimed steps: mesh-static tables, first allocations, size history
            place(k)
            torch.cuda.synchronize()
            s0 = _lib.sync_count()
            t0 = time.perf_counter()
            info = {}
            out = cfx.run_step(body, key=key, info=info) if sync_free else body()
            torch.cuda.synchronize()
            if k >= 0:
                times.append(1e3 * (time.perf_counter() - t0))
                passes.append(info.get("passes", 1))
                syncs.append(_lib.sync_count() - s0)
                nnz.append(out.A.nnz)
            del out
        return dict(ms_per_step=sum(times) / len(times), ms_each=[round(t, 3) for t in times], passes=passes,
                    read_backs_per_step=sum(syncs) / len(syncs), nnz_first_last=[nnz[0], nnz[-1]])
    a = run(True, f"moving-{n}")
    state["cd"] = None
    bb = run(False, f"moving-{n}-rb")
    return {"what": f"moving sphere, centre advanced by {shift_h} h per step, {nsteps} timed steps, full rebuild of plan and "
                    "sparsity every step (the reference rebuilds too: cut.cpp:845-868); the level-set update itself is "
                    "outside the timed region",
            "mesh": n, "sync_free": a, "sizes_read_back": bb,
            "incremental_sparsity": "config_p2_gyroid_256.moving_domain",
            "incremental_note": "the P1 pattern of this workload is a masked copy of the mesh-static stencil (no hash sets: "
                                "6.1 ms for 378 M entries, 0.9 of it for the hashed rows next to the interface), so nothing is kept "
                                "from the previous step here; rows are reused where patterns are hashed (degree 2 / vector "
                                "spaces): measured on the moving gyroid of config_p2_gyroid_256 (DESIGN.md 3, round 4)"}


def projected_scaling(torch, device, n, order, one_gpu_ms, worlds=(2, 4, 8)):
    """PROJECTION, not a measurement: every rank's slab of the N-rank owner-computes partition timed one after the
    other on this one GPU with the halo level-set values already in place (no exchange, no RCCL): the slowest rank
    bounds the N-GPU step from below.  No scaling curve over real GPUs exists until the driver's 8-GPU run."""
    import gc

    from cutfemx_amd import _lib
    from cutfemx_amd.dist import DistributedPoisson, SlabPartition
    out = {}
    for world in worlds:
        per_rank = []
        for r in range(world):
            part = SlabPartition.create_owner(n, world, r)
            dp = DistributedPoisson(part, device, order=order, mode="owner")
            dp.part.world = 1            # skip the exchange: the analytic halo values are already in place
            for _ in range(2):
                dp.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(4):
                dp.step()
            torch.cuda.synchronize()
            per_rank.append(round(1e3 * (time.perf_counter() - t0) / 4, 3))
            del dp
            gc.collect(); _lib.release_cache(); torch.cuda.empty_cache()
        out[str(world)] = dict(slowest_rank_ms=max(per_rank), per_rank_ms=per_rank,
                               projected_speedup=one_gpu_ms / max(per_rank))
    # the exchange of a step, bounded from above on this one GPU: an interior rank sends 2 level-set planes to and
    # receives 2 from each of its two neighbours; staged through pinned host memory (what the gloo rehearsal transport
    # does) that is 4 device -> host and 4 host -> device copies of one plane pair each, one after the other.  RCCL
    # send / recv over xGMI (no host hop, both directions at once) is expected well below it.
    ps = (n + 1) ** 2
    planes = torch.zeros(2 * ps, device=device, dtype=torch.float64)
    host = torch.empty(2 * ps, dtype=torch.float64).pin_memory()
    xs = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _nb in range(2):
            host.copy_(planes, non_blocking=True)
            torch.cuda.synchronize()
            planes.copy_(host, non_blocking=True)
            torch.cuda.synchronize()
        xs.append(1e3 * (time.perf_counter() - t0))
    exchange_ms = sorted(xs)[len(xs) // 2]
    # ... and what the same bytes cost when they only have to be MOVED on the device (a device-to-device copy of the four
    # plane pairs): a floor for any transport.  An xGMI link carries ~50 GB/s per direction (MI355X_MICROARCH.md: 7 links
    # x ~153 GB/s bidirectional per GPU), both neighbours on their own links: bytes / 50 GB/s + ~30 us of launch as the
    # labelled ESTIMATE in between.
    other = torch.empty_like(planes)
    ds = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _nb in range(2):
            other.copy_(planes); planes.copy_(other)
        torch.cuda.synchronize()
        ds.append(1e3 * (time.perf_counter() - t0))
    device_copy_ms = sorted(ds)[len(ds) // 2]
    xgmi_estimate_ms = 1e3 * (2 * 8 * ps) / 50e9 + 0.03
    for w in out.values():
        w["projected_speedup_with_exchange"] = one_gpu_ms / (w["slowest_rank_ms"] + exchange_ms)
        w["projected_speedup_xgmi_estimate"] = one_gpu_ms / (w["slowest_rank_ms"] + xgmi_estimate_ms)
    return dict(kind="projection from one GPU (each rank's slab run alone); NOT a measured scaling curve",
                one_gpu_ms=one_gpu_ms, by_world=out, exchange_upper_bound_ms=round(exchange_ms, 4),
                exchange_device_copy_ms=round(device_copy_ms, 4), exchange_xgmi_estimate_ms=round(xgmi_estimate_ms, 4),
                exchange_xgmi_estimate_is="one neighbour's two planes at 50 GB/s per direction of one xGMI link + 30 us; an "
                                          "ESTIMATE, nothing was sent",
                exchange_upper_bound_is="level-set halo of an interior rank (2 vertex planes to and from each of two "
                                        f"neighbours, {2 * 2 * 8 * ps / 1e6:.1f} MB each way) staged through pinned host memory on "
                                        "this one GPU, copies one after the other, added to the slowest rank's step with no "
                                        "overlap; the N-GPU job moves it with RCCL send / recv over xGMI")


LINE_LIMIT = 4096      # the driver's parser lost round 4's 20 kB line: the contract line stays far below that


def _r(v, digits=4):
    """Number rounded to `digits` significant digits (None stays None)."""
    if v is None or isinstance(v, (bool, str)):
        return v
    return float(f"{float(v):.{digits}g}")


def _phase_summary(leg):
    """One-number summaries of a secondary configuration: step time and, per priced phase, the fraction of the HBM
    roofline on algorithmic bytes and counter traffic / algorithmic bytes."""
    if not isinstance(leg, dict):
        return None
    if "error" in leg:
        return {"error": str(leg["error"])[:120]}
    s = {"ms_per_step": _r(leg.get("ms_per_step"))}
    for key, short in (("roofline", "matrix"), ("roofline_sparsity", "sparsity")):
        r = leg.get(key)
        if r:
            s[short] = {"ms": _r(r.get("phase_ms")), "frac": _r(r.get("frac")),
                        "traffic_ratio": _r(r["traffic"] / r["algorithmic_bytes"]) if r.get("traffic") else None}
    md = leg.get("moving_domain")
    if isinstance(md, dict) and "incremental" in md:
        s["moving_create_matrix_ms"] = {"incremental": md["incremental"].get("create_matrix_ms"),
                                        "full": md["full_rebuild"].get("create_matrix_ms"),
                                        "reused_share": md["incremental"].get("reused_share")}
    if "step_mode" in leg:
        s["step_mode"] = leg["step_mode"]
    if isinstance(leg.get("as_one_step"), dict):
        s["as_one_step"] = {k: leg["as_one_step"].get(k) for k in ("ms_per_step", "read_backs", "passes")}
    return s


def headline_line(out):
    """The ONE stdout line of the contract: the driver's fields, `roofline`, `cpu_baseline` and one-number summaries of
    the secondary legs, under LINE_LIMIT bytes.  Everything else is in bench_detail.json (`emit`)."""
    line = {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")}
    r = out.get("roofline")
    if r:
        line["roofline"] = {"bound": r["bound"], "achieved": _r(r.get("achieved")), "peak": r["peak"], "unit": r["unit"],
                            "frac": _r(r.get("frac")), "traffic": r.get("traffic"), "kernel": r.get("kernel"),
                            "avg_launch_us": _r(r.get("avg_launch_us")),
                            "algorithmic_bytes_per_launch": r.get("algorithmic_bytes_per_launch")}
    else:
        line["roofline"] = None
    c = out.get("cpu_baseline")
    if c:
        line["cpu_baseline"] = {"value": _r(c["value"]), "unit": c["unit"], "cores": c["cores"], "kind": c["kind"],
                                "sample": str(c["sample"])[:300], "seconds": _r(c.get("seconds")),
                                "extrapolated_to_workload_s": _r(c.get("seconds_at_512_extrapolated"))}
    else:
        line["cpu_baseline"] = None
    ca = out.get("cpu_baseline_all_cores")
    if ca:
        line["cpu_baseline_all_cores"] = {"value": _r(ca["value"]), "cores": ca["cores"], "kind": ca["kind"]}
    w = out.get("whole_step_roofline")
    if w:
        line["whole_step"] = {"frac_survey_bytes": _r(w.get("frac_survey_bytes")), "frac_moved_bytes": _r(w.get("frac_moved_bytes"))}
    sm = out.get("step_mode")
    if sm:
        line["step_mode"] = {k: sm.get(k) for k in ("sync_free", "passes", "read_backs_per_step", "launches_per_step")}
    if out.get("phases_ms"):
        line["phases_ms"] = {k: _r(v) for k, v in out["phases_ms"].items()}
    if out.get("cut_quadrature_points_per_s"):
        line["cut_quadrature_points_per_s"] = _r(out["cut_quadrature_points_per_s"])
    if out.get("multi_gpu"):
        mg = out["multi_gpu"]
        line["multi_gpu"] = {k: mg.get(k) for k in ("transport", "rccl_ranks", "world", "slowest_rank_ms_per_step",
                                                    "imbalance", "exchange_ms", "per_rank_ms_per_step")}
    sec = {}
    for name in ("config_128", "config_32"):
        if isinstance(out.get(name), dict):
            sec[name] = {"ms_per_step": _r(out[name].get("ms_per_step"))} if "error" not in out[name] else {"error": out[name]["error"][:120]}
    for name in ("config_p2_gyroid_256", "config_elasticity_share"):
        if out.get(name) is not None:
            sec[name] = _phase_summary(out[name])
    if isinstance(out.get("implicit_structured"), dict):
        sec["implicit_structured"] = {"ms_per_step": _r(out["implicit_structured"].get("ms_per_step"))}
    md = out.get("moving_domain")
    if isinstance(md, dict):
        sec["moving_domain"] = ({"error": md["error"][:120]} if "error" in md else
                                {"sync_free_ms": _r(md["sync_free"]["ms_per_step"]),
                                 "sizes_read_back_ms": _r(md["sizes_read_back"]["ms_per_step"]),
                                 "read_backs_per_step": md["sync_free"].get("read_backs_per_step")})
    ps = out.get("projected_scaling")
    if isinstance(ps, dict):
        if "error" in ps:
            sec["projected_scaling"] = {"error": ps["error"][:120]}
        else:
            w8 = ps["by_world"].get("8") or {}
            sec["projected_scaling"] = {"kind": "projection from one GPU, NOT a measured curve",
                                        "slowest_rank_ms_at_8": w8.get("slowest_rank_ms"),
                                        "speedup_at_8_no_exchange": _r(w8.get("projected_speedup")),
                                        "speedup_at_8_with_exchange": _r(w8.get("projected_speedup_with_exchange")),
                                        "speedup_at_8_xgmi_estimate": _r(w8.get("projected_speedup_xgmi_estimate"))}
    if sec:
        line["secondary"] = sec
    line["detail"] = out.get("detail_file")
    text = json.dumps(line, separators=(",", ":"))
    # never let an optional summary push the contract line over the limit
    for drop in ("secondary", "phases_ms", "cpu_baseline_all_cores", "step_mode", "whole_step"):
        if len(text) < LINE_LIMIT:
            break
        line.pop(drop, None)
        text = json.dumps(line, separators=(",", ":"))
    return text


def emit(out):
    """Write the full record to bench_detail.json (gpurun_out/ when that directory can be made, next to bench.py
    otherwise) and to stderr (`# bench_detail: ...`); print the contract line -- alone -- on stdout."""
    target = None
    name = os.environ.get("CFX_BENCH_DETAIL", "bench_detail.json")     # (profiling scripts name their own copy)
    for d in (ROOT / "gpurun_out", ROOT):
        try:
            d.mkdir(exist_ok=True)
            (d / name).write_text(json.dumps(out, indent=1))
            target = str((d / name).relative_to(ROOT))
            break
        except OSError:
            continue
    out["detail_file"] = target
    # (stdout carries the contract line and nothing else: whatever cut round 4's record short -- a cap on the head or
    # on the tail of the captured stdout -- cannot reach a single line of ~2.5 kB.  The full record goes to stderr.)
    if os.environ.get("CFX_BENCH_PRINT_DETAIL", "1") != "0":
        sys.stderr.write("# bench_detail: " + json.dumps(out) + "\n")
        sys.stderr.flush()
    print(headline_line(out), flush=True)


def main():
    args = parse()
    if args.cpu_worker:
        cpu_slab_worker(*args.cpu_worker)
        return
    if args.dump_outputs and args.gpus != 1:
        raise SystemExit("--dump-outputs writes the outputs of a one-GPU step: run it with --gpus 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args))
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: cutfemx_amd has no CPU fallback")
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch N>1 as `python -m torch.distributed.run "
                         f"--nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 bench.py --gpus {args.gpus} ...`")
    # rehearsal on a one-GPU box: CFX_REHEARSE=1 puts every rank on cuda:0 and uses gloo
    # (RCCL cannot place two ranks on one device); never set on the real multi-GPU run
    rehearse = os.environ.get("CFX_REHEARSE") == "1"
    if rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)
            # a scaling line must be an xGMI line: without CFX_REHEARSE, an RCCL communicator that does not come up on
            # every rank moves its device buffers through this nccl group instead ('rccl-torch'); a host-staged gloo fallback
            # ends the job (cutfemx_amd.dist.TransportError)
            os.environ.setdefault("CFX_DIST_STRICT", "1")
    os.environ["CFX_DEVICE"] = str(local_rank)
    # One explicit HIP stream for torch and the engine alike (CFX_BENCH_STREAM=0: the legacy null stream, the library's
    # default).  Dependent launches on the null stream are ~10 us apart on this stack (rocprofv3 kernel trace,
    # profiles/r04_launch_gaps.txt, taken when a step had 73 of them; 52 now: `step_mode.launches_per_step`).
    if os.environ.get("CFX_BENCH_STREAM", "1") != "0":
        from cutfemx_amd import _lib as _sl
        bench_stream = torch.cuda.Stream(device)
        torch.cuda.set_stream(bench_stream)
        _sl.check(_sl.lib().cfx_set_stream(C.c_void_p(bench_stream.cuda_stream)))

    n = args.n
    # one step on a tiny mesh first: HIP initialisation and the loading of the library's code objects happen here and
    # not inside the first step of the workload, whose time then is table building + first allocation
    tw = time.perf_counter()
    if world == 1:
        measure(8, 1, 0, args.order, 1, 0, device, profile=False)
    torch.cuda.synchronize()
    library_warmup_ms = 1e3 * (time.perf_counter() - tw)
    m = measure(n, args.steps, args.warmup, args.order, world, rank, device, profile=args.full,
                dump_dir=args.dump_outputs)
    if m.get("setup") is not None:
        m["setup"]["library_warmup_ms"] = library_warmup_ms
    out = {
        "metric": "assembled DOFs/sec (active dofs / full hot-path step) + cut-quadrature points/sec, "
                  "Poisson P1 sphere level-set",
        "value": m["value"], "unit": "DOF/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": m["ms_per_step"],
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": f"3D Poisson P1, sphere level set on {n}^3 background mesh ({6 * n ** 3} tets), "
                               f"Nitsche + ghost penalty, runtime quadrature order {args.order}; one step = cut + "
                               "rules + sparsity + assemble_matrix + assemble_vector + deactivation",
                   "cells": 6 * n ** 3, "active_dofs": m["active_dofs"],
                   "parallelism": "1 gpu" if world == 1 else (
                       f"z-slabs x{world} weighted by active cells, owner computes (halo 1+2 layers), RCCL p2p "
                       "level-set halo" if os.environ.get("CFX_DIST_MODE", "owner") == "owner" else
                       f"z-slabs x{world} weighted by active cells, halo 3 layers, RCCL p2p row reduction")},
    }
    for k in ("cut_quadrature_points_per_s", "cut_quadrature_points_reference_equivalent", "assemble_matrix_dofs_per_s",
              "counts", "step_mode", "multi_gpu", "phases_ms", "setup", "memory", "kernels", "roofline", "roofline_by_kernel", "roofline_longest_kernel",
              "whole_step_roofline"):
        out[k] = m.get(k)
    if not args.full:
        # a plain run: the result line and nothing else (no extra legs, no detail file)
        if rank == 0:
            print(headline_line(out), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    if rank == 0 and world == 1:
        if not args.no_secondary and n != 128:
            s = measure(128, 20, 3, args.order, 1, 0, device, profile=False)
            out["config_128"] = {"workload": "configs[1]: 128^3 background mesh, same form", "value": s["value"],
                                 "unit": "DOF/s", "ms_per_step": s["ms_per_step"], "active_dofs": s["active_dofs"]}
        if not args.no_secondary and n != 32:
            # the launch-bound end of the same step: 32^3 (configs[0]-sized), where the step is ~40 kernel floors
            try:
                s = measure(32, 200, 10, args.order, 1, 0, device, profile=True)
                sm = s.get("step_mode") or {}
                out["config_32"] = {"workload": "32^3 background mesh, same form (launch-bound)", "value": s["value"], "unit": "DOF/s",
                                    "ms_per_step": s["ms_per_step"], "active_dofs": s["active_dofs"],
                                    "launches_per_step": sm.get("launches_per_step"),
                                    "read_backs_per_step": sm.get("read_backs_per_step")}
            except Exception as e:
                out["config_32"] = {"error": f"{type(e).__name__}: {e}"}
        if not args.no_secondary:
            import gc
            from cutfemx_amd import _lib as _cl
            gc.collect(); torch.cuda.empty_cache(); _cl.release_cache()
            for name, fn in (("config_p2_gyroid_256", secondary_p2_gyroid), ("config_elasticity_share", secondary_elasticity_share)):
                try:
                    out[name] = fn(torch, device)
                except Exception as e:      # (e.g. not enough free HBM): reported, never silently dropped
                    out[name] = {"error": f"{type(e).__name__}: {e}"}
                gc.collect(); torch.cuda.empty_cache(); _cl.release_cache()
        if not args.no_secondary:
            # "implicit-structured" variant (report both): on the generated box mesh the
            # classification derives the Kuhn connectivity from the cube index instead of streaming 12.9 GB of it.
            # Opt-in (CFX_IMPLICIT_BOX=1), identical domain array; the headline `value` stays on explicit connectivity.
            os.environ["CFX_IMPLICIT_BOX"] = "1"
            try:
                im = measure(n, max(3, args.steps // 2), 2, args.order, 1, 0, device)
                k = (im.get("kernels") or {}).get("classify_box")
                cells = 6 * n ** 3
                alg = float(cells + (n + 1) ** 3)   # 1 B domain code out per cell + the 1 B sign code of every vertex once
                out["implicit_structured"] = {
                    "what": "same step, classification from the generated mesh's cube index (no connectivity stream)",
                    "value": im["value"], "unit": "DOF/s", "ms_per_step": im["ms_per_step"],
                    "classify_box_us": None if not k else k["avg_us"],
                    "classify_box_algorithmic_bytes": alg,
                    "classify_box_achieved_GBs": None if not k else alg / (k["avg_us"] * 1e-6) / 1e9}
            finally:
                os.environ.pop("CFX_IMPLICIT_BOX", None)
        if not args.no_secondary:
            try:
                import gc
                from cutfemx_amd import _lib as _cl
                gc.collect(); torch.cuda.empty_cache(); _cl.release_cache()
                out["moving_domain"] = moving_domain_leg(torch, device, n, args.order)
                gc.collect(); torch.cuda.empty_cache(); _cl.release_cache()
            except Exception as e:
                out["moving_domain"] = {"error": f"{type(e).__name__}: {e}"}
        if not args.no_secondary:
            try:
                out["projected_scaling"] = projected_scaling(torch, device, n, args.order, m["ms_per_step"])
            except Exception as e:
                out["projected_scaling"] = {"error": f"{type(e).__name__}: {e}"}
        out["cpu_baseline"] = None if args.no_cpu else cpu_baseline(args.cpu_n, args.order)
        out["cpu_baseline_all_cores"] = None if args.no_cpu else cpu_baseline_all_cores(args.cpu_n, args.order)
    elif rank == 0:
        # the same bounded CPU sample as the one-GPU line, timed on rank 0's host cores after the timed region (the
        # other ranks wait in destroy_process_group)
        out["cpu_baseline"] = None if args.no_cpu else cpu_baseline(args.cpu_n, args.order)
    if rank == 0:
        emit(out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
