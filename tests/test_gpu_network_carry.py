"""RELP_CARRY_NETWORK: the basis of a network LP kept as a spanning forest of the rows (network_carry.hip).

Every value on both sides of the parity tests is an integer below 2^53 (B^-1 has entries in {0, +-1}; costs and capacities
are integers), so the forest carry and the explicit carry agree with ``==``, pivot for pivot."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import relp_amd  # noqa: E402
from relp_amd.api import CARRY_EXPLICIT, CARRY_NETWORK, ERR_ARGUMENT, RATIO_HARRIS, RATIO_TEXTBOOK, RelpError  # noqa: E402
from relp_oracle.network import adjacency_from_rows  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_FLOW_ROWS = [[0, 0, 0, 0], [2, 0, 0, 0], [1, 1, 0, 0], [0, 1, 2, 0]]
SHORTEST_PATH_ROWS = [[0, 0, 0, 0], [1, 0, 0, 0], [2, 2, 0, 0], [0, 3, 1, 0]]


def arc_list(arcs):
    return [(a, b, v) for a, outgoing in enumerate(arcs) for b, v in outgoing]


def graph(nr_vertices, nr_arcs, drop_into_s=True):
    from relp_amd.workloads import max_flow_graph
    tail, head, value = max_flow_graph(nr_vertices, nr_arcs)
    if drop_into_s:  # the reference's objective is the gross flow out of s: equal to the max flow without these arcs
        keep = (head != 0) & (tail != nr_vertices - 1)
        tail, head, value = tail[keep], head[keep], value[keep]
    return tail, head, value


def scipy_max_flow(nr_vertices, tail, head, capacity):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_flow
    g = csr_matrix((capacity.astype(np.int32), (tail, head)), shape=(nr_vertices, nr_vertices))
    return maximum_flow(g, 0, nr_vertices - 1).flow_value


def max_flow_model(nr_vertices, tail, head, capacity):
    return relp_amd.Model.max_flow(nr_vertices, list(zip(tail.tolist(), head.tolist(), capacity.tolist())), 0, nr_vertices - 1)


def shortest_path_model(nr_vertices, tail, head, length):
    return relp_amd.Model.shortest_path(nr_vertices, list(zip(tail.tolist(), head.tolist(), length.tolist())), 0, nr_vertices - 1)


def test_the_examples_certified_exactly():
    model = relp_amd.Model.max_flow(4, arc_list(adjacency_from_rows(MAX_FLOW_ROWS)), 0, 3)
    solver = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1, certify=1).load_model(model)
    result = solver.solve_relaxation()
    assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
    assert solver.record()["carry"] == "network"
    assert Fraction(solver.objective_exact()) == -3
    assert np.allclose(solver.solution(), [2, 1, 1, 1, 2], atol=1e-9)
    exact = dict(solver.solution_exact())
    assert [Fraction(exact.get(j, 0)) for j in range(5)] == [2, 1, 1, 1, 2]
    exact = dict(solver.solution_exact(original=True))
    assert [Fraction(exact.get(j, 0)) for j in range(5)] == [2, 1, 1, 1, 2]
    model = relp_amd.Model.shortest_path(4, arc_list(adjacency_from_rows(SHORTEST_PATH_ROWS)), 0, 3)
    solver = relp_amd.Solver(carry=CARRY_NETWORK, certify=1).load_model(model)
    result = solver.solve_relaxation()
    assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
    assert Fraction(solver.objective_exact()) == 3
    exact = dict(solver.solution_exact())
    assert [Fraction(exact.get(j, 0)) for j in range(5)] == [0, 1, 0, 0, 1]


def _models(nr_vertices, nr_arcs):
    tail, head, value = graph(nr_vertices, nr_arcs)
    return [("max_flow", max_flow_model(nr_vertices, tail, head, value), {"implicit_bounds": 1}),
            ("shortest_path", shortest_path_model(nr_vertices, tail, head, value), {})]


@pytest.mark.parametrize("nr_vertices,nr_arcs", [(256, 1000), (2304, 9000), (10000, 40000)])
def test_pivot_for_pivot_against_the_explicit_carry(nr_vertices, nr_arcs):
    for name, model, extra in _models(nr_vertices, nr_arcs):
        a = relp_amd.Solver(carry=CARRY_EXPLICIT, **extra).load_model(model)
        b = relp_amd.Solver(carry=CARRY_NETWORK, **extra).load_model(model)
        rule = RATIO_TEXTBOOK if a.m <= 8192 else RATIO_HARRIS
        a.close()
        b.close()
        a = relp_amd.Solver(carry=CARRY_EXPLICIT, ratio_rule=rule, **extra).load_model(model)
        b = relp_amd.Solver(carry=CARRY_NETWORK, ratio_rule=rule, **extra).load_model(model)
        a.begin_phase_one()
        b.begin_phase_one()
        pivots = 0
        for phase in (1, 2):
            if phase == 2:
                a.begin_phase_two()
                b.begin_phase_two()
            while True:
                da, ra = a.iterate(1)
                db, rb = b.iterate(1)
                assert (da, ra) == (db, rb), (name, pivots)
                if da == 0:
                    break
                assert a.last_pivot() == b.last_pivot(), (name, pivots)
                if pivots < 200:
                    assert np.array_equal(a.b(), b.b()), (name, pivots)
                    ga, gb = a.gamma(), b.gamma()
                    assert np.array_equal(np.isnan(ga), np.isnan(gb)) and np.array_equal(ga[~np.isnan(ga)], gb[~np.isnan(gb)]), (name, pivots)
                pivots += 1
            if phase == 1 and a.objective_function_value() != 0.0:
                break
        assert a.objective_function_value() == b.objective_function_value(), name
        assert pivots > 0
        a.close()
        b.close()


def test_the_carry_operations_equal_a_dense_solve():
    nr_vertices = 40
    tail, head, value = graph(nr_vertices, 120)
    model = shortest_path_model(nr_vertices, tail, head, value)
    solver = relp_amd.Solver(carry=CARRY_NETWORK).load_model(model)
    m = solver.m
    arcs = list(zip(tail.tolist(), head.tolist()))
    arcs.sort()

    def column(c):  # the device LP's column: provider arc c, or artificial -1-k (unit column of its row)
        out = np.zeros(m)
        if c < 0:
            return None
        t, h = arcs[c]
        if t != 0:
            out[t - 1] -= 1.0
        if h != 0:
            out[h - 1] += 1.0
        return out

    rng = np.random.default_rng(7)
    solver.begin_phase_one()
    checked = 0
    for step in range(40):
        basis = solver.basis()
        B = np.zeros((m, m))
        artificial_rows = [r for r in range(m)]
        for k, c in enumerate(basis):
            col = column(c)
            if col is None:  # artificials: the unit column of the row they were created for (phase-one rows in order)
                col = np.zeros(m)
                col[artificial_rows[-1 - c]] = 1.0
            B[:, k] = col
        v = rng.integers(-3, 4, size=m).astype(float)
        rows = np.arange(m, dtype=np.int32)
        assert np.allclose(solver.left_multiply_by_basis_inverse(rows, v), np.linalg.solve(B, v))
        assert np.allclose(solver.right_multiply_by_basis_inverse(rows, v), np.linalg.solve(B.T, v))
        r = int(rng.integers(0, m))
        assert np.allclose(solver.basis_inverse_row(r), np.linalg.solve(B.T, np.eye(m)[r]))
        checked += 1
        done, _ = solver.iterate(3)
        if done == 0:
            break
    assert checked >= 2


def _random_max_flow(rng, nr_vertices, nr_arcs):
    nr_arcs = min(nr_arcs, (nr_vertices - 1) ** 2 - (nr_vertices - 2))  # the arcs that neither enter s nor leave t
    pairs = set()
    while len(pairs) < nr_arcs:
        t, h = (int(x) for x in rng.integers(0, nr_vertices, size=2))
        if t != h and h != 0 and t != nr_vertices - 1:  # nothing into s, nothing out of t: the objective is the max flow
            pairs.add((t, h))
    arcs = sorted((t, h, int(rng.integers(1, 8))) for t, h in pairs)
    return np.array([a[0] for a in arcs]), np.array([a[1] for a in arcs]), np.array([a[2] for a in arcs])


def test_certificate_with_complemented_basic_arcs():
    """Small max-flow LPs whose optimum needs flow cancelled: arcs leave the basis at their capacity and come back in while held
    complemented, so optimal bases hold complemented basic arcs.  The forest certificate must agree with scipy's max flow and,
    value for value, with the general certificate of the explicit carry; the exact flow must respect capacities and conservation."""
    checked = 0
    for trial in (26, 169, 174, 248, 7, 11):  # (the first four reach such bases from one start or both)
        rng = np.random.default_rng(trial)
        nr_vertices = int(rng.integers(8, 40))
        tail, head, capacity = _random_max_flow(rng, nr_vertices, int(rng.integers(2 * nr_vertices, 5 * nr_vertices)))
        expected = scipy_max_flow(nr_vertices, tail, head, capacity)
        model = max_flow_model(nr_vertices, tail, head, capacity)
        for crash in (0, 1):
            tree = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1, certify=1, crash=crash).load_model(model)
            explicit = relp_amd.Solver(carry=CARRY_EXPLICIT, implicit_bounds=1, certify=1, crash=crash).load_model(model)
            rt, re = tree.solve_relaxation(), explicit.solve_relaxation()
            assert rt.kind == re.kind == relp_amd.FINITE_OPTIMUM, trial
            assert rt.certified and re.certified, (trial, crash)
            assert Fraction(tree.objective_exact()) == Fraction(explicit.objective_exact()) == -expected, (trial, crash)
            exact = tree.solution_exact()
            flow = [exact.get(j, Fraction(0)) for j in range(len(tail))]
            assert all(0 <= f <= int(c) for f, c in zip(flow, capacity)), (trial, crash)
            net = [Fraction(0)] * nr_vertices
            for f, t, h in zip(flow, tail.tolist(), head.tolist()):
                net[h] += f
                net[t] -= f
            assert all(v == 0 for v in net[1:-1]) and net[-1] == expected, (trial, crash)
            assert np.allclose(tree.solution(), [float(f) for f in flow], atol=1e-9)
            assert exact == explicit.solution_exact(), (trial, crash)
            tree.close()
            explicit.close()
            checked += 1
    assert checked == 12


def test_textbook_rule_beyond_8192_rows():
    """The forest carry has the reference's ratio rule at every size: AUTO resolves to it on integer data beyond 8192 rows (the
    explicit carry falls back to Harris there), and the optimum is scipy's max flow, certified."""
    nr_vertices = 10000
    tail, head, capacity = graph(nr_vertices, 40000)
    expected = scipy_max_flow(nr_vertices, tail, head, capacity)
    model = max_flow_model(nr_vertices, tail, head, capacity)
    for rule in (None, RATIO_TEXTBOOK):
        extra = {} if rule is None else {"ratio_rule": rule}
        solver = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1, certify=1, **extra).load_model(model)
        assert solver.m > 8192
        result = solver.solve_relaxation()
        record = solver.record()
        assert record["ratio_rule"] == "textbook"
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        assert Fraction(solver.objective_exact()) == -expected
        # price, path, the ratio test across workgroups (three kernels), update, re-hang: seven per pivot, one budget per batch
        assert record["kernel_launches"] >= 7 * (result.pivots_phase_one + result.pivots_phase_two)
        solver.close()


def test_forest_statistics_per_pivot():
    from relp_amd.api import SW_NETWORK_STATS
    nr_vertices = 2304
    tail, head, capacity = graph(nr_vertices, 9000)
    model = max_flow_model(nr_vertices, tail, head, capacity)
    plain = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1).load_model(model)
    counted = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1, switches=SW_NETWORK_STATS).load_model(model)
    rp, rc = plain.solve_relaxation(), counted.solve_relaxation()
    assert (rp.pivots_phase_one, rp.pivots_phase_two, rp.objective) == (rc.pivots_phase_one, rc.pivots_phase_two, rc.objective)
    assert "network_tree" not in plain.record()
    stats = counted.record()["network_tree"]
    assert 0 < stats["pivots"] <= rc.pivots_phase_one + rc.pivots_phase_two
    assert 1 <= stats["depth_mean"] <= stats["depth_max"] <= counted.m
    assert 1 <= stats["subtree_mean"] <= stats["subtree_max"] <= counted.m
    assert 1 <= stats["path_mean"] <= stats["path_max"] <= counted.m
    plain.close()
    counted.close()


def _check_flow(solver, nr_vertices, tail, head, capacity, expected):
    flow = solver.solution()
    order = np.lexsort((head, tail))
    t_sorted, h_sorted, c_sorted = tail[order], head[order], capacity[order]
    assert np.all(flow >= -1e-9) and np.all(flow <= c_sorted + 1e-9)
    net = np.zeros(nr_vertices)
    np.add.at(net, h_sorted, flow)
    np.subtract.at(net, t_sorted, flow)
    assert np.max(np.abs(net[1:-1])) <= 1e-6


@pytest.mark.parametrize("crash", [0, 1])
def test_config5_full_size(crash):
    nr_vertices, nr_arcs = 65536, 1048576
    tail, head, capacity = graph(nr_vertices, nr_arcs, drop_into_s=False)
    expected = scipy_max_flow(nr_vertices, tail, head, capacity)
    model = max_flow_model(nr_vertices, tail, head, capacity)
    solver = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1, certify=1, crash=crash).load_model(model)
    result = solver.solve_relaxation()
    assert result.kind == relp_amd.FINITE_OPTIMUM
    assert abs(result.objective + expected) <= 1e-9 * expected
    assert result.certified == 1 and Fraction(solver.objective_exact()) == -expected
    _check_flow(solver, nr_vertices, tail, head, capacity, expected)
    record = solver.record()
    assert record["carry"] == "network"
    assert record["device_bytes"] < 2e9
    assert result.solve_seconds < 30
    solver.close()


def test_beyond_the_explicit_carry():
    nr_vertices, nr_arcs = 262144, 2097152
    tail, head, capacity = graph(nr_vertices, nr_arcs, drop_into_s=False)
    expected = scipy_max_flow(nr_vertices, tail, head, capacity)
    model = max_flow_model(nr_vertices, tail, head, capacity)
    solver = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1, certify=1, crash=1).load_model(model)
    result = solver.solve_relaxation()
    assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
    assert Fraction(solver.objective_exact()) == -expected
    assert result.solve_seconds < 120
    solver.close()


def test_shortest_path_12k_vertices_and_no_path():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    nr_vertices = 12000
    tail, head, weight = graph(nr_vertices, 60000, drop_into_s=False)
    g = csr_matrix((weight.astype(np.float64), (tail, head)), shape=(nr_vertices, nr_vertices))
    expected = dijkstra(g, directed=True, indices=0)[nr_vertices - 1]
    solver = relp_amd.Solver(carry=CARRY_NETWORK, certify=1).load_model(shortest_path_model(nr_vertices, tail, head, weight))
    result = solver.solve_relaxation()
    assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
    assert Fraction(solver.objective_exact()) == expected
    # no s-t path: nothing enters the target
    keep = head != nr_vertices - 1
    model = shortest_path_model(nr_vertices, tail[keep], head[keep], weight[keep])
    result = relp_amd.Solver(carry=CARRY_NETWORK).load_model(model).solve_relaxation()
    assert result.kind == relp_amd.INFEASIBLE


def test_rejects_lps_that_are_not_networks():
    path = os.path.join(ROOT, "data", "netlib", "AFIRO.SIF")
    with pytest.raises(RelpError) as info:
        relp_amd.Solver(carry=CARRY_NETWORK).load_mps(path)
    assert info.value.status == ERR_ARGUMENT and "column" in str(info.value)
    model = relp_amd.Model.max_flow(4, arc_list(adjacency_from_rows(MAX_FLOW_ROWS)), 0, 3)
    with pytest.raises(RelpError) as info:
        relp_amd.Solver(carry=CARRY_NETWORK).load_model(model)
    assert info.value.status == ERR_ARGUMENT and "implicit_bounds" in str(info.value)
