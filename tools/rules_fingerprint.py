#!/usr/bin/env python3
"""One SHA-256 per array of every rule set the engine makes on a fixed list of small cases: two builds of the engine
(CFX_LIB names the library, as for the other variant tools) that print the same lines compute the same bits.
usage: [CFX_LIB=build/libcfx_<name>.so] python tools/rules_fingerprint.py [--inputs-only] [--per-case] > out.txt
--per-case prints one SHA-256 per case (over its array lines, in order) and one over all lines instead of the lines
themselves: the form of profiles/rules_refactor_fingerprint.json.

Cases: cell hosts -- every mesh of tests/exact_cut.CASES, "phi<0" / "phi>0" / "phi=0" at orders 1..4 as single calls,
the ["phi<0", "phi=0"] pair through runtime_quadratures at order 2, full_cell_rules on the cut cells; several level sets
-- the meshes and SELECTORS of tests/test_gpu_multi_level_set.py at orders 1 and 3; facet hosts -- the HOST_CASES of
tests/test_gpu_exact_moments.py with the same selectors and orders, full_facet_rules, and both through to_cells on every
side.  On every rule set: physical points; on every cell-hosted one (the to_cells images of the facet-hosted ones
included; the evaluators take cell reference points) normals and level-set values.
Before anything runs, the inputs are checked to contain every cut sign mask (bit v: phi < 0 at vertex v of the host):
1..6 on 2-D cells and triangle hosts, 1..14 on 3-D cells, 1 and 2 on segment hosts.  --inputs-only stops there (no GPU).
A tool and not a test: a compiler upgrade may move bits legitimately."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import exact_cut as X
from helpers import level_set_values, scrambled_mesh
from oracle import pyoracle as O
from test_gpu_exact_moments import HOST_CASES
from test_gpu_multi_level_set import SELECTORS as MULTI_SELECTORS, second_level_set

SELECTORS = ("phi<0", "phi>0", "phi=0")
ORDERS = (1, 2, 3, 4)
MULTI_MESHES = [(2, 24, False), (3, 10, False), (2, 16, True), (3, 8, True)]  # the fixture of test_gpu_multi_level_set.py


def cut_masks(phi, hosts):
    """Sign masks of the cut hosts (rows of vertex ids): not all values < 0 and not all > 0."""
    v = phi[hosts]
    cut = ~(np.all(v < 0, axis=1) | np.all(v > 0, axis=1))
    return set(((v[cut] < 0).astype(np.int64) << np.arange(hosts.shape[1])).sum(axis=1).tolist())


def require_masks(group, nv, seen):
    want = set(range(1, (1 << nv) - 1))
    assert want <= seen, f"{group}: cut sign masks {sorted(want - seen)} do not occur in the cases"
    print(f"# {group}: all {len(want)} cut sign masks present", file=sys.stderr)


LINES = []  # "<group>/<case>/<rule set>/<array> <sha256>"


def report():
    if "--per-case" not in sys.argv:
        print("\n".join(LINES))
        return
    digest = lambda lines: hashlib.sha256("\n".join(lines).encode()).hexdigest()
    cases = {}
    for l in LINES:
        cases.setdefault("/".join(l.split("/")[:2]), []).append(l)
    for case, lines in cases.items():
        print(f"{case} arrays {len(lines)} {digest(lines)}")
    print(f"all arrays {len(LINES)} {digest(LINES)}")


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def emit(key, R, cd=None, nls=1):
    import cutfemx_amd as cfx
    arrays = dict(points=R.points, weights=R.weights, offsets=R.offsets, parent_map=R.parent_map,
                  physical_points=R.physical_points)
    if R.host_width:
        arrays["host_rows"] = R.host_rows
        arrays["host_verts"] = R._get("host_verts", R._view.host_verts, R.num_rules * (R.tdim + 1), np.int32)
    elif cd is not None and R.total_points > 0:
        for ls in range(nls):
            arrays[f"normals{ls}"] = cfx.normal(cd, R, ls)
            arrays[f"values{ls}"] = cfx.level_set_value(cd, R, ls)
    for name, a in arrays.items():
        LINES.append(f"{key}/{name} {sha(a)}")


def main():
    O.build()
    cases = {name: X.build_case(O, name) for name in X.CASES}
    multi = []
    for tdim, n, scr in MULTI_MESHES:
        om = scrambled_mesh(O, tdim, n) if scr else O.mesh_box(tdim, n)
        multi.append((f"{tdim}d-n{n}{'-scrambled' if scr else ''}", tdim, om,
                      [level_set_values(om.x, tdim), second_level_set(om.x, tdim)]))
    hosts = {(name, which): X.host_case(O, name, which) for name, which in HOST_CASES}
    for tdim in (2, 3):
        require_masks(f"cell hosts {tdim}-D", tdim + 1,
                      set().union(*(cut_masks(cs["phi"], cs["conn"]) for cs in cases.values() if cs["tdim"] == tdim)))
        require_masks(f"several level sets {tdim}-D", tdim + 1,
                      set().union(*(cut_masks(phis[0], om.conn) for _, d, om, phis in multi if d == tdim)))
        require_masks("segment hosts" if tdim == 2 else "triangle hosts", tdim,
                      set().union(*(cut_masks(cases[name]["phi"], hc["verts"]) for (name, _), hc in hosts.items()
                                    if cases[name]["tdim"] == tdim)))
    if "--inputs-only" in sys.argv:
        return
    import cutfemx_amd as cfx

    for name, cs in cases.items():
        mesh = cfx.Mesh.from_arrays(cs["tdim"], cs["x"], cs["conn"])
        f = cfx.Function(cfx.FunctionSpace(mesh, 1), cs["phi"].copy())
        cd = cfx.cut(f)
        for sel in SELECTORS:
            for order in ORDERS:
                emit(f"cell/{name}/{sel}/o{order}", cfx.runtime_quadrature(cd, sel, order), cd)
        for sel, R in cfx.runtime_quadratures(cd, ["phi<0", "phi=0"], 2).items():
            emit(f"cell/{name}/pair/{sel}/o2", R, cd)
        emit(f"cell/{name}/full/o2", cfx.full_cell_rules(mesh, cs["cut"], 2), cd)
    for name, tdim, om, phis in multi:
        mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
        V = cfx.FunctionSpace(mesh, 1)
        cd = cfx.cut([cfx.Function(V, p.copy()) for p in phis])
        for sel in MULTI_SELECTORS:
            for order in (1, 3):
                emit(f"multi/{name}/{sel}/o{order}", cfx.runtime_quadrature(cd, sel, order), cd, 2)
    for (name, which), hc in hosts.items():
        cs = cases[name]
        tdim = cs["tdim"]
        mesh = cfx.Mesh.from_arrays(tdim, cs["x"], cs["conn"])
        f = cfx.Function(cfx.FunctionSpace(mesh, 1), cs["phi"].copy())
        cdc = cfx.cut(f)  # the cell-hosted cut of the same level set: what the evaluators take
        rows = cfx.exterior_facets(mesh) if which == "exterior" else \
            cfx.interior_facets_for_cells(mesh, np.arange(cs["conn"].shape[0], dtype=np.int32))
        assert np.array_equal(rows.rows, hc["rows"])
        cd = cfx.cut(f, rows, tdim - 1)
        sets = [(f"{sel}/o{order}", cfx.runtime_quadrature(cd, sel, order)) for sel in SELECTORS for order in ORDERS]
        sets += [(f"full-{sel}/o2", cfx.full_facet_rules(cd, sel, 2)) for sel in (None, "phi<0")]
        for tag, R in sets:
            emit(f"facet/{name}-{which}/{tag}", R)
            for side in range(R.host_width // 2):
                emit(f"facet/{name}-{which}/{tag}/side{side}", R.to_cells(side), cdc)
    report()


if __name__ == "__main__":
    main()
