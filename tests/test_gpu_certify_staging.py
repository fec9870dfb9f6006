"""What a handle keeps between its certificates (relp_amd/csrc/certify.hip, `CertifyScratch`): the pinned staging arena the uploads
are packed into and the digits come back into, the host thread of the dual lifting, and witnesses that are only finished when they
are first asked for.  None of it may change a result, leak into another handle, or outlive its handle (``-m gpu``).

Exact objectives: tests/golden/<NAME>.json holds the rationals (the oracle's); tests/golden/netlib_expected.json holds Netlib's
decimal values with their tolerances, which the same strings must also meet.  The witnesses are judged by relp_amd/witness.py:
exact substitution with `fractions.Fraction` on the host, no call into the library."""
import json
import os
import threading
from fractions import Fraction

import pytest

import relp_amd
from relp_amd import WITNESS_DUAL, WITNESS_PRIMAL, WITNESS_RAY
from relp_amd.witness import check_infeasible, check_optimum, check_unbounded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = json.load(open(os.path.join(ROOT, "tests", "golden", "netlib_expected.json")))
NAMES = ["AFIRO", "SC50A"]


def netlib(name):
    return relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF"))


def golden_objective(name):
    return Fraction(json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))["objective"])


def certified_objective(solver, name):
    result = solver.solve_relaxation()
    assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1, (name, result.kind, result.certified)
    text = solver.objective_exact()
    assert Fraction(text) == golden_objective(name), (name, text)
    assert abs(float(Fraction(text)) - EXPECTED[name]["expected"]) <= EXPECTED[name]["tolerance"] * max(1.0, abs(EXPECTED[name]["expected"])), name
    return text


@pytest.mark.parametrize("name", NAMES)
def test_certified_twice_on_one_handle(name):
    """The second certificate finds the arena, the second stream and the worker thread of the first."""
    solver = relp_amd.Solver(certify=1).load_model(netlib(name))
    try:
        first = certified_objective(solver, name)
        x_first = solver.solution_exact()
        second = certified_objective(solver, name)
        assert first == second and solver.solution_exact() == x_first
    finally:
        solver.close()


def test_two_handles_from_two_threads():
    """Each handle has its own arena and worker: certificates of two handles run at the same time."""
    models = {name: netlib(name) for name in NAMES}
    solvers = {name: relp_amd.Solver(certify=1).load_model(models[name]) for name in NAMES}
    out, errors = {}, []

    def run(name):
        try:
            texts = [certified_objective(solvers[name], name) for _ in range(2)]
            out[name] = (texts, solvers[name].witness_exact(WITNESS_PRIMAL), solvers[name].witness_exact(WITNESS_DUAL))
        except BaseException as error:  # noqa: BLE001  (reported by the main thread)
            errors.append((name, error))

    threads = [threading.Thread(target=run, args=(name,)) for name in NAMES]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for name in NAMES:
            texts, x, y = out[name]
            assert texts[0] == texts[1]
            check_optimum(models[name], x, y, Fraction(texts[0]))
    finally:
        for solver in solvers.values():
            solver.close()


def small(kinds, columns, b, variables):
    return relp_amd.Model.from_general_form(columns, kinds, b, variables)


def test_infeasible_and_unbounded_2_by_2_are_certified_with_witnesses():
    # x + y <= 1 and x + y >= 2: infeasible
    infeasible = small(["Less", "Greater"], [[(0, 1), (1, 1)], [(0, 1), (1, 1)]], [1, 2], [(1, 0, None), (1, 0, None)])
    # min -x - y with x - y <= 1 and -x + y <= 1: unbounded along (1, 1)
    unbounded = small(["Less", "Less"], [[(0, 1), (1, -1)], [(0, -1), (1, 1)]], [1, 1], [(-1, 0, None), (-1, 0, None)])
    for model, kind in ((infeasible, relp_amd.INFEASIBLE), (unbounded, relp_amd.UNBOUNDED)):
        solver = relp_amd.Solver(certify=1).load_model(model)
        try:
            for _ in range(2):  # (a second solve on the handle: new witnesses, the old ones are gone)
                result = solver.solve_relaxation()
                assert result.kind == kind and result.certified == 1, (kind, result.kind, result.certified)
                if kind == relp_amd.INFEASIBLE:
                    check_infeasible(model, solver.witness_exact(WITNESS_DUAL), Fraction(solver.objective_exact()))
                else:
                    assert solver.objective_exact() == "-inf"
                    check_unbounded(model, solver.witness_exact(WITNESS_PRIMAL), solver.witness_exact(WITNESS_RAY))
        finally:
            solver.close()


@pytest.mark.parametrize("name", NAMES)
def test_witnesses_are_finished_on_demand(name):
    """Read only after another accessor, read twice, in both orders, and again after a second solve: the same values, and they
    prove the optimum by exact substitution."""
    model = netlib(name)
    solver = relp_amd.Solver(certify=1).load_model(model)
    try:
        text = certified_objective(solver, name)
        structural = solver.solution_exact()          # an accessor before any witness is asked for
        assert Fraction(solver.objective_exact()) == Fraction(text)
        y = solver.witness_exact(WITNESS_DUAL)        # the dual first: the primal is shared with the kept exact solution
        x = solver.witness_exact(WITNESS_PRIMAL)
        assert solver.witness_exact(WITNESS_DUAL) == y and solver.witness_exact(WITNESS_PRIMAL) == x  # the second read scales nothing again
        check_optimum(model, x, y, Fraction(text))
        assert structural == {j: v for j, v in x.items() if j < model.nr_structural}
        assert certified_objective(solver, name) == text
        x_again = solver.witness_exact(WITNESS_PRIMAL)  # the other order after the second solve
        y_again = solver.witness_exact(WITNESS_DUAL)
        assert (x_again, y_again) == (x, y)
        check_optimum(model, x_again, y_again, Fraction(text))
    finally:
        solver.close()


def test_a_handle_closed_without_asking_for_witnesses():
    """The worker thread is joined and the arena freed by close(); a handle that never certified has neither."""
    for _ in range(2):  # (the runtime's and the big-integer pool's threads, made once per process, exist after these)
        solver = relp_amd.Solver(certify=1).load_model(netlib("AFIRO"))
        certified_objective(solver, "AFIRO")
        solver.close()
    idle = relp_amd.Solver(certify=1).load_model(netlib("AFIRO"))
    idle.close()
    # the process' count of threads does not grow with the handles that came and went
    counts = []
    for _ in range(4):
        solver = relp_amd.Solver(certify=1).load_model(netlib("AFIRO"))
        certified_objective(solver, "AFIRO")
        solver.close()
        counts.append(len(os.listdir("/proc/self/task")))
    assert counts[-1] <= counts[0], counts
