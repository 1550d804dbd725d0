"""The cell-local arithmetic of the reinitialisation (cutfemx_amd/csrc/cfx_reinit_cell.h) on the GPU, one lane per
case, against the independent references of tests/reinit_exact.py: the cases and the assertions are those of
tests/reinit_cell_cases.py, which tests/test_reinit_cell_reference.py applies to the same header on the CPU and to the
numpy model.  The GPU contracts multiplications and additions, so its figures differ from the CPU's in detail.

tests/cpp/reinit_cell_probe.hip is compiled once, with the compiler, the architecture and the flags of the engine's
Makefile, and started once for the whole module under a time limit.  If that child fails, dies on a signal or runs into
its limit, every test of the module fails without another start."""
import subprocess

import pytest

import reinit_cell_cases as C

pytestmark = pytest.mark.gpu

_lost = []


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    if _lost:
        pytest.fail("the probe is not started again: " + _lost[0], pytrace=False)
    work = tmp_path_factory.mktemp("reinit_cell_probe")
    try:
        exe = C.compile_program("reinit_cell_probe.hip", work / "reinit_cell_probe", offload=True)
        return C.run_program(exe, work, seconds=90.0)
    except (AssertionError, subprocess.TimeoutExpired) as e:
        _lost.append(str(e)[:3000])
        pytest.fail(_lost[0], pytrace=False)


@pytest.mark.parametrize("name", ["well3", "well2", "boundary3", "boundary2"])
def test_update_well_shaped_and_boundary(results, name):
    C.check_tight(name, results[0][name], "gpu")


@pytest.mark.parametrize("name", ["flat3", "flat2"])
def test_update_graded_flatness(results, name):
    C.check_flat(name, results[0][name], "gpu")
    print(C.error_table(name, {"gpu": results[0][name], "model": C.model_update(name)}))


@pytest.mark.parametrize("dim", [2, 3])
def test_near_field(results, dim):
    C.check_seed(dim, *results[1][dim], "gpu")
