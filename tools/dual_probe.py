"""What the dual simplex saves on a re-solve after cuts, and what one of its pivots costs (a real MI355X; not a test).

For the cut cases of tests/dual_lps.py at m = 1025 and m = 2049 (the parent solved cold and certified, 24 cuts its vertex violates):
  cold       a cold certified solve of the child: ms, pivots
  dual       ``solve_dual`` from the parent's basis, certified: ms, dual pivots, primal clean-up pivots
  per pivot  wall time of ``iterate_dual(256)`` over the pivots it made, beside ``iterate(256)`` of the primal loop from the slack
             basis on the same handle -- as the handle runs it (fused pivot or three kernels, replayed from a graph) and as three
             kernels in plain launches, which is the form the dual loop has (five plain launches).  Every call ends in a stream
             synchronise, so these are times a caller sees, launch overhead included.
  device     the same without the host: the dual batch between two events on the handle's stream (``dual_device_seconds`` of
             ``record()``: five kernels per pivot and the gaps between them), and the kernels of a primal pivot one by one inside
             the running loop (``relp_profile_kernel``: pricing + ratio test / fused pivot + update, their sum, no gaps).
``--decimal`` divides every matrix value by 10: the Harris rule runs instead of the reference's.
Every figure is the median of 5 runs after one warm-up, in one process.

``--start`` prints the other table instead, one line per child (4 and 24 cuts, integer and decimal data): how the dual loop starts.
  solve_dual        wall time of the whole call around a stream synchronise, and how much of it ``begin_dual`` took
                    (``dual_start_seconds`` of ``record()``)
  begin_dual        from scratch: ``dual_start_seconds`` and ``dual_start_gemms``
  begin_dual_from   from the inverse of the parent's handle, which stays open beside the child's: the same two, and the guard's residual
  solve_dual_from   the whole call with that start
with the smallest and largest of the 5 runs beside each median.  Run against a library that has no ``relp_begin_dual_from``
(``RELP_AMD_LIB``), it prints ``solve_dual`` alone.

``--pricing 0 1`` prints the third table, one line per child (the same eight) and leaving-row rule (``Options.dual_pricing``: 0 largest
infeasibility, 1 steepest edge), both rules in the one run: the dual pivots of ``solve_dual``, the device time of one of them
(``dual_device_seconds`` over the pivots: the batches between two events, the weight pass of rule 1 included), and the wall time of
``solve_dual`` and of ``solve_dual_from`` around a stream synchronise.

``--bounded``: the child of a branching step on an LP with a bound on every structural variable (tests/dual_bounded_lps.py, 24 cuts and
8 tightened bounds unless ``--cuts`` says otherwise), re-solved both ways from the same basis of the formulation: ``solve_dual`` with
the bounds as rows (``implicit_bounds=0``) and ``solve_dual_bounded`` on implicit bounds (``implicit_bounds=1``).  Per way: the rows of
the device LP, the dual pivots, the wall time of the call and the device time per dual pivot; where the row limit of the dual loop
refuses the explicit formulation, the refusal.  Both end at the same exact objective.

``--bounded --long-step``: the same child on implicit bounds under both ratio tests from the same basis, the plain one and the
long-step (bound-flipping) one (``Solver.set_dual_long_step``), a line per rule: dual pivots, flips, the whole certified call and the
device time per dual pivot.  ``--every N`` puts a bound on every N-th structural variable (1 unless given; 2 is the family of the
tests), ``--tight N`` tightens N bounds (8 unless given): with few bounds the walks of the two rules coincide and the difference of
the two device times is what a pivot with the switch on and no flip costs.

``--bounded --start``: how the loop on implicit bounds starts, the columns of ``--start`` for the children of ``--bounded`` and, at each
size, for a pure branch (no cut, 8 tightened bounds: the child has the parent's rows).  The parent's handle stays open beside the
child's, solved cold on the device, so it holds its basis at its own positions and some basic columns complemented.
  begin_dual_bounded        from scratch: ``dual_start_seconds`` and ``dual_start_gemms``
  begin_dual_bounded_from   from the parent's inverse: the same two, the guard's residual, and how many inherited positions were
                            complemented on one side only / not the parent's (``dual_inherit_complemented``, ``dual_inherit_moved``)
  solve_dual_bounded, solve_dual_bounded_from   the whole certified call, and how much of it the start took
``--traced`` as with ``--start``: the two begin calls only, plain launches, for a run under rocprofv3 --kernel-trace.

``--farkas``: an INFEASIBLE child at each size, without bounds (``dual_lps.infeasible_child``: two contradicting rows over two variables
that are positive at the parent's vertex) and on implicit bounds (a bound on every variable; the branch fixes two of them at 0 and a row
asks for their sum to be at least 1, as ``dual_bounded_lps.infeasible_child`` builds it), a line per way to the verdict:
  dual        ``solve_dual`` / ``solve_dual_bounded`` with ``farkas=True``, certified: the whole call, its start, the dual pivots and
              ``certify_seconds`` (one launch of the leaving-row kernel, one modular inverse, one transposed lifting, the exact products)
  inherited   the same through ``solve_dual_from`` / ``solve_dual_bounded_from``, the parent's handle open beside the child's
  cold        ``solve_relaxation`` of the child on a fresh handle: ms, pivots and whether the verdict came back certified (on implicit
              bounds it does not: ``collect_result`` certifies finite optima only there)
Run against a library without ``relp_set_dual_farkas`` (``RELP_AMD_LIB``), it prints the cold lines alone.

``--cutoff``: the child of the first table (24 cuts) and, with a bound on every structural variable, the child of ``--bounded`` (24 cuts,
8 tightened bounds), integer and decimal data, each re-solved twice from the same basis in the same run, a line per way:
  full       ``solve_dual`` / ``solve_dual_bounded`` to the certified optimum, the switch off: the whole call, the dual pivots,
             ``certify_seconds`` and the device time per dual pivot
  cutoff     the same call under ``cutoff=`` halfway between the parent's optimum and the child's (both from the runs without it): the
             whole call, the dual pivots, ``certify_seconds`` (the proof of the bound: one modular inverse, one transposed lifting, the
             exact products) and in how many of the 5 runs the proof failed (decimal data: under the Harris rule a relative cost may be
             negative by less than ``tol_dual``, and a column without a bound cannot absorb that)
Run against a library without ``relp_set_dual_cutoff`` (``RELP_AMD_LIB``), it prints the full lines alone.

    python tools/dual_probe.py [--sizes 1025 2049] [--decimal] [--cuts N] [--start [--traced]] [--pricing 0 1] [--bounded [--long-step | --start [--traced]]] [--farkas] [--cutoff]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, path)
import relp_amd  # noqa: E402
import dual_lps  # noqa: E402

RUNS = 5


def median_of(run):
    run()  # warm-up
    samples = [run() for _ in range(RUNS)]
    return [statistics.median(column) for column in zip(*samples)]


def probe(m, decimal, n_cuts):
    seed, default_cuts = dual_lps.STATE_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts or default_cuts, decimal=decimal)
    parent = relp_amd.Solver(certify=1).load_model(case.parent)
    assert parent.solve_relaxation().certified
    child, basis, _ = case.child(parent.basis(), parent.solution_exact())
    parent.close()
    solver = relp_amd.Solver(certify=1).load_model(child)
    plain = relp_amd.Solver(certify=0, pivot_kernels=1, use_graph=0).load_model(child)

    def cold():
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        return 1e3 * (result.solve_seconds + result.certify_seconds), result.pivots_phase_one + result.pivots_phase_two, solver.objective_exact()

    def dual():
        result = solver.solve_dual(basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        return 1e3 * (result.solve_seconds + result.certify_seconds), solver.dual_pivots(), result.pivots_phase_two, solver.objective_exact()

    def dual_pivot():
        solver.begin_dual(basis)
        started = time.perf_counter()
        done, _ = solver.iterate_dual(256)
        return (1e6 * (time.perf_counter() - started) / max(1, done), done)

    def dual_device():
        solver.begin_dual(basis)
        done, _ = solver.iterate_dual(256)
        return (1e6 * solver.record()["dual_device_seconds"] / max(1, done),)

    def primal_kernels(handle, kernels):
        def run():
            handle.begin_phase_one()
            handle.iterate(64)
            return tuple(1e6 * handle.profile_kernel(which, 64) for which in kernels)
        return run

    def primal_pivot(handle):
        def run():
            handle.begin_phase_one()
            started = time.perf_counter()
            done, _ = handle.iterate(256)
            return (1e6 * (time.perf_counter() - started) / max(1, done), done)
        return run

    exact = {cold()[2], dual()[3]}
    assert len(exact) == 1, exact
    cold_ms, cold_pivots = median_of(lambda: cold()[:2])
    dual_ms, dual_pivots, clean_up = median_of(lambda: dual()[:3])
    dual_us, dual_done = median_of(dual_pivot)
    primal_us, _ = median_of(primal_pivot(solver))
    plain_us, _ = median_of(primal_pivot(plain))
    plan = child.kernel_path()
    (dual_device_us,) = median_of(dual_device)
    own_kernels = median_of(primal_kernels(solver, (0, 1) if plan["fused"] else (0, 1, 2)))
    plain_kernels = median_of(primal_kernels(plain, (0, 1, 2)))
    print("m = %d + %d cuts (%s, %s): cold %.1f ms, %d pivots | solve_dual %.1f ms, %d dual + %d primal pivots | per pivot: dual %.1f us "
          "(%d pivots), primal %.1f us as the handle runs it, %.1f us as three kernels in plain launches | device time per pivot: dual %.1f us, "
          "primal kernels %s = %.1f us as the handle runs it, %s = %.1f us as three kernels" % (
              m, child.nr_rows - m, "decimal" if decimal else "integer", "fused pivot" if plan["fused"] else "three-kernel pivot", cold_ms, cold_pivots,
              dual_ms, dual_pivots, clean_up, dual_us, dual_done, primal_us, plain_us, dual_device_us,
              " + ".join("%.1f" % v for v in own_kernels), sum(own_kernels), " + ".join("%.1f" % v for v in plain_kernels), sum(plain_kernels)))
    solver.close()
    plain.close()


def spread_of(run):
    """Median, minimum and maximum of each column over the 5 runs after the warm-up."""
    run()
    samples = [run() for _ in range(RUNS)]
    return [(statistics.median(column), min(column), max(column)) for column in zip(*samples)]


def start_probe(m, decimal, n_cuts, traced=False):
    """One child of the table of DESIGN.md section 10: how the dual loop starts and what that is of the whole re-solve.  ``traced``:
    the two begin calls only, every handle with plain launches."""
    seed, _ = dual_lps.STATE_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts, decimal=decimal)
    options = dict(certify=1, use_graph=0) if traced else dict(certify=1)
    parent = relp_amd.Solver(**options).load_model(case.parent)
    assert parent.solve_relaxation().certified
    child, basis, _ = case.child(parent.basis(), parent.solution_exact())
    solver = relp_amd.Solver(**options).load_model(child)
    inherits = hasattr(relp_amd.lib(), "relp_begin_dual_from")  # (a library of before the start from the parent's inverse: solve_dual alone)

    def solve(call):
        def run():
            started = time.perf_counter()
            result = call()
            wall = 1e3 * (time.perf_counter() - started)
            assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
            record = solver.record()
            return wall, 1e3 * record.get("dual_start_seconds", 0.0), solver.dual_pivots()
        return run

    def begin(call):
        def run():
            call()
            record = solver.record()
            return 1e3 * record["dual_start_seconds"], record["dual_start_gemms"], record["dual_start_residual"] or 0.0
        return run

    label = "m = %d + %d cuts, %s" % (m, n_cuts, "decimal" if decimal else "integer")
    if traced:
        (scratch_ms, _, _), (scratch_gemms, _, _), _ = spread_of(begin(lambda: solver.begin_dual(basis)))
        (from_ms, _, _), (from_gemms, _, _), _ = spread_of(begin(lambda: solver.begin_dual_from(parent, basis)))
        print("%s (traced, plain launches): begin_dual %.2f ms, %d GEMMs | begin_dual_from %.2f ms, %d GEMMs" % (label, scratch_ms, scratch_gemms, from_ms, from_gemms), flush=True)
        solver.close()
        parent.close()
        return
    (solve_ms, solve_lo, solve_hi), (start_in_solve, _, _), (pivots, _, _) = spread_of(solve(lambda: solver.solve_dual(basis)))
    text = "%s: solve_dual %.1f ms (%.1f .. %.1f), %d dual pivots" % (label, solve_ms, solve_lo, solve_hi, pivots)
    if inherits:
        (scratch_ms, scratch_lo, scratch_hi), (scratch_gemms, _, _), _ = spread_of(begin(lambda: solver.begin_dual(basis)))
        (from_ms, from_lo, from_hi), (from_gemms, _, _), (residual, _, _) = spread_of(begin(lambda: solver.begin_dual_from(parent, basis)))
        (warm_ms, warm_lo, warm_hi), _, (warm_pivots, _, _) = spread_of(solve(lambda: solver.solve_dual_from(parent, basis)))
        # (the two inverses differ in their last bits, so on dual-degenerate data the two walks need not make the same pivots)
        text += (", of which begin_dual %.1f ms = %.0f %% | begin_dual %.2f ms (%.2f .. %.2f), %d GEMMs | begin_dual_from %.2f ms (%.2f .. %.2f), "
                 "%d GEMMs, guard's residual %.1e | solve_dual_from (%s) %.1f ms (%.1f .. %.1f), %d dual pivots" % (
                     start_in_solve, 100.0 * start_in_solve / solve_ms, scratch_ms, scratch_lo, scratch_hi, scratch_gemms, from_ms, from_lo, from_hi,
                     from_gemms, residual, solver.record()["dual_start"], warm_ms, warm_lo, warm_hi, warm_pivots))
    print(text, flush=True)
    solver.close()
    parent.close()


def pricing_probe(m, decimal, n_cuts, rules):
    """One child of the pricing table of DESIGN.md section 10, a line per rule."""
    seed, _ = dual_lps.STATE_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts, decimal=decimal)
    parent = relp_amd.Solver(certify=1).load_model(case.parent)
    assert parent.solve_relaxation().certified
    child, basis, _ = case.child(parent.basis(), parent.solution_exact())
    objectives = set()
    for rule in rules:
        solver = relp_amd.Solver(certify=1, dual_pricing=rule).load_model(child)

        def solve(call):
            def run():
                started = time.perf_counter()
                result = call()
                wall = 1e3 * (time.perf_counter() - started)
                assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
                objectives.add(solver.objective_exact())
                pivots = solver.dual_pivots()
                return wall, pivots, 1e6 * solver.record()["dual_device_seconds"] / max(1, pivots), result.pivots_phase_two
            return run

        (wall, lo, hi), (pivots, _, _), (device_us, _, _), (clean_up, _, _) = spread_of(solve(lambda: solver.solve_dual(basis)))
        (from_wall, from_lo, from_hi), (from_pivots, _, _), (from_us, _, _), _ = spread_of(solve(lambda: solver.solve_dual_from(parent, basis)))
        print("m = %d + %d cuts, %s, %s: %d dual + %d primal pivots, %.1f us of device time per dual pivot | solve_dual %.1f ms (%.1f .. %.1f) | "
              "solve_dual_from %.1f ms (%.1f .. %.1f), %d dual pivots, %.1f us each" % (
                  m, n_cuts, "decimal" if decimal else "integer", "steepest edge" if rule else "largest infeasibility", pivots, clean_up, device_us,
                  wall, lo, hi, from_wall, from_lo, from_hi, from_pivots, from_us), flush=True)
        solver.close()
    assert len(objectives) == 1, objectives  # every run, under either rule, ends at the same exact optimum
    parent.close()


def bounded_probe(m, decimal, n_cuts, n_tight=8):
    """One child of the bounded table of DESIGN.md section 10, a line per formulation."""
    import dual_bounded_lps
    case = dual_bounded_lps.BoundedCase(m, 1000 + m, n_cuts, n_tight, decimal=decimal, every=1)
    parent = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(case.parent.model)
    assert parent.solve_relaxation().certified
    child, basis, _, branches = case.child(parent.basis(), parent.solution_exact())
    parent.close()
    label = "m = %d + %d cuts, %d tightened bounds, %s" % (m, n_cuts, len(branches), "decimal" if decimal else "integer")
    objectives = set()
    for implicit, entry in ((0, "solve_dual"), (1, "solve_dual_bounded")):
        refusal = child.model.dual_bounded_refusal(implicit_bounds=implicit)
        rows = child.model.kernel_path(implicit_bounds=implicit)["m"]
        if refusal:
            print("%s | %s, implicit_bounds = %d: %d rows, refused: %s" % (label, entry, implicit, rows, refusal), flush=True)
            continue
        solver = relp_amd.Solver(certify=1, implicit_bounds=implicit).load_model(child.model)

        def run():
            started = time.perf_counter()
            result = getattr(solver, entry)(basis)
            wall = 1e3 * (time.perf_counter() - started)
            assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
            objectives.add(solver.objective_exact())
            pivots = solver.dual_pivots()
            return wall, pivots, 1e6 * solver.record()["dual_device_seconds"] / max(1, pivots), result.pivots_phase_two, 1e3 * solver.record()["dual_start_seconds"]

        (wall, lo, hi), (pivots, _, _), (device_us, us_lo, us_hi), (clean_up, _, _), (start_ms, _, _) = spread_of(run)
        print("%s | %s, implicit_bounds = %d: %d rows, %d dual + %d primal pivots, %.1f ms (%.1f .. %.1f) of which the start %.1f ms, "
              "%.1f us (%.1f .. %.1f) of device time per dual pivot" % (label, entry, implicit, rows, pivots, clean_up, wall, lo, hi, start_ms, device_us, us_lo, us_hi),
              flush=True)
        solver.close()
    assert len(objectives) <= 1, objectives  # both formulations end at the same exact optimum


def bounded_start_probe(m, decimal, n_cuts, n_tight=8, traced=False):
    """One child of the table "the inherited start on implicit bounds" of DESIGN.md section 10.  ``n_cuts = 0``: a pure branch."""
    import dual_bounded_lps
    case = dual_bounded_lps.BoundedCase(m, 1000 + m, n_cuts, n_tight, decimal=decimal, every=1)
    options = dict(certify=1, implicit_bounds=1, use_graph=0) if traced else dict(certify=1, implicit_bounds=1)
    parent = relp_amd.Solver(**options).load_model(case.parent.model)
    assert parent.solve_relaxation().certified
    child, basis, _, branches = case.child(parent.basis(), parent.solution_exact())
    assert child.m == m + n_cuts
    solver = relp_amd.Solver(**options).load_model(child.model)
    label = "m = %d + %d cuts, %d tightened bounds, %s" % (m, n_cuts, len(branches), "decimal" if decimal else "integer")
    objectives = set()

    def solve(call):
        def run():
            started = time.perf_counter()
            result = call()
            wall = 1e3 * (time.perf_counter() - started)
            assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
            objectives.add(solver.objective_exact())
            return wall, 1e3 * solver.record()["dual_start_seconds"], solver.dual_pivots()
        return run

    def begin(call):
        def run():
            call()
            record = solver.record()
            return (1e3 * record["dual_start_seconds"], record["dual_start_gemms"], record["dual_start_residual"] or 0.0,
                    record["dual_inherit_complemented"], record["dual_inherit_moved"])
        return run

    (scratch_ms, scratch_lo, scratch_hi), (scratch_gemms, _, _), _, _, _ = spread_of(begin(lambda: solver.begin_dual_bounded(basis)))
    (from_ms, from_lo, from_hi), (from_gemms, _, _), (residual, _, _), (complemented, _, _), (moved, _, _) = spread_of(
        begin(lambda: solver.begin_dual_bounded_from(parent, basis)))
    how = solver.record()["dual_start"]
    text = "%s | begin_dual_bounded %.2f ms (%.2f .. %.2f), %d GEMMs | begin_dual_bounded_from (%s) %.2f ms (%.2f .. %.2f), %d GEMMs, guard's residual %.1e, %d complemented, %d moved" % (
        label, scratch_ms, scratch_lo, scratch_hi, scratch_gemms, how, from_ms, from_lo, from_hi, from_gemms, residual, complemented, moved)
    if not traced:
        (cold_ms, cold_lo, cold_hi), (cold_start, _, _), (cold_pivots, _, _) = spread_of(solve(lambda: solver.solve_dual_bounded(basis)))
        (warm_ms, warm_lo, warm_hi), (warm_start, _, _), (warm_pivots, _, _) = spread_of(solve(lambda: solver.solve_dual_bounded_from(parent, basis)))
        text += (" | solve_dual_bounded %.1f ms (%.1f .. %.1f), of which the start %.1f ms = %.0f %%, %d dual pivots | solve_dual_bounded_from %.1f ms (%.1f .. %.1f), "
                 "of which the start %.2f ms = %.1f %%, %d dual pivots" % (cold_ms, cold_lo, cold_hi, cold_start, 100.0 * cold_start / cold_ms, cold_pivots,
                                                                       warm_ms, warm_lo, warm_hi, warm_start, 100.0 * warm_start / warm_ms, warm_pivots))
        assert len(objectives) == 1, objectives  # either start ends at the same exact optimum
    print(text, flush=True)
    solver.close()
    parent.close()


def long_step_probe(m, decimal, n_cuts, n_tight, every):
    """One child of the long-step table of DESIGN.md section 10, a line per ratio test."""
    import dual_bounded_lps
    case = dual_bounded_lps.BoundedCase(m, 1000 + m, n_cuts, n_tight, decimal=decimal, every=every)
    parent = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(case.parent.model)
    assert parent.solve_relaxation().certified
    child, basis, _, branches = case.child(parent.basis(), parent.solution_exact())
    parent.close()
    label = "m = %d + %d cuts, %d tightened bounds, a bound on every %d. variable, %s" % (m, n_cuts, len(branches), every, "decimal" if decimal else "integer")
    objectives = set()
    for long_step in (False, True):
        solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
        solver.set_dual_long_step(long_step)

        def run():
            started = time.perf_counter()
            result = solver.solve_dual_bounded(basis)
            wall = 1e3 * (time.perf_counter() - started)
            assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
            objectives.add(solver.objective_exact())
            record, pivots = solver.record(), solver.dual_pivots()
            assert record["dual_long_step"] is long_step
            return wall, pivots, 1e6 * record["dual_device_seconds"] / max(1, pivots), result.pivots_phase_two, record["dual_flips"], record["dual_long_step_skipped"]

        (wall, lo, hi), (pivots, _, _), (device_us, us_lo, us_hi), (clean_up, _, _), (flips, _, _), (skipped, _, _) = spread_of(run)
        print("%s | %s: %d dual + %d primal pivots, %d flips (%d pivots fell back), %.1f ms (%.1f .. %.1f), %.1f us (%.1f .. %.1f) of device time per dual pivot" % (
            label, "long step" if long_step else "plain rule", pivots, clean_up, flips, skipped, wall, lo, hi, device_us, us_lo, us_hi), flush=True)
        solver.close()
    assert len(objectives) == 1, objectives  # both rules end at the same exact optimum


def farkas_probe(m, bounded):
    """One child of the table "the INFEASIBLE verdict, proved" of DESIGN.md section 10, a line per way to the verdict."""
    from fractions import Fraction
    proves = hasattr(relp_amd.lib(), "relp_set_dual_farkas")  # (a library of before the proof: the cold solve alone)
    if bounded:
        import dual_bounded_lps
        case = dual_bounded_lps.BoundedCase(m, 1000 + m, 0, 0, every=1)
        form = case.parent
        options = dict(certify=1, implicit_bounds=1)
        parent = relp_amd.Solver(**options).load_model(form.model)
        assert parent.solve_relaxation().certified
        vertex = {int(j): v for j, v in parent.solution_exact().items() if j < form.ns}
        j, k = [v for v in sorted(vertex) if vertex[v] > 0 and form.upper[v] is not None][:2]
        columns, upper = [list(column) for column in form.columns], list(form.upper)
        for variable in (j, k):
            columns[variable].append((form.m, Fraction(1)))
            upper[variable] = 0
        child_form = dual_bounded_lps.Formulation(columns, list(form.b) + [1], form.cost, upper, n_greater=1)
        child, basis = child_form.model, dual_bounded_lps.extended_basis(form, child_form, parent.basis())
        entries = ("solve_dual_bounded", "solve_dual_bounded_from")
    else:
        seed, _ = dual_lps.STATE_CASES[m]
        case = dual_lps.cut_case(m, dual_lps.MIXED, seed, 0)
        options = dict(certify=1)
        parent = relp_amd.Solver(**options).load_model(case.parent)
        assert parent.solve_relaxation().certified
        child, basis = dual_lps.infeasible_child(case, parent.basis(), parent.solution_exact())
        entries = ("solve_dual", "solve_dual_from")
    label = "m = %d, %s, infeasible child of %d rows on the device" % (m, "implicit bounds" if bounded else "no bounds", child.kernel_path(**options)["m"])
    solver = relp_amd.Solver(**options).load_model(child)
    values = set()

    def dual(call):
        def run():
            started = time.perf_counter()
            result = call()
            wall = 1e3 * (time.perf_counter() - started)
            assert result.kind == relp_amd.INFEASIBLE and result.certified, relp_amd.lib().relp_last_error(solver._h).decode()
            values.add(solver.objective_exact())
            return wall, 1e3 * solver.record()["dual_start_seconds"], solver.dual_pivots(), 1e3 * result.certify_seconds
        return run

    def cold():
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.INFEASIBLE
        return 1e3 * (result.solve_seconds + result.certify_seconds), result.pivots_phase_one + result.pivots_phase_two, 1e3 * result.certify_seconds, result.certified

    if proves:
        for entry, call in ((entries[0], lambda: getattr(solver, entries[0])(basis, farkas=True)),
                            (entries[1], lambda: getattr(solver, entries[1])(parent, basis, farkas=True))):
            (wall, lo, hi), (start_ms, _, _), (pivots, _, _), (certify_ms, certify_lo, certify_hi) = spread_of(dual(call))
            print("%s | %s (%s): %.1f ms (%.1f .. %.1f), of which the start %.2f ms, %d dual pivots, the proof %.2f ms (%.2f .. %.2f), y'b = %s" % (
                label, entry, solver.record()["dual_start"], wall, lo, hi, start_ms, pivots, certify_ms, certify_lo, certify_hi, sorted(values)), flush=True)
    (cold_ms, cold_lo, cold_hi), (cold_pivots, _, _), (cold_certify, _, _), (certified, _, _) = spread_of(cold)
    print("%s | cold solve_relaxation: %.1f ms (%.1f .. %.1f), %d pivots, certificate %.2f ms, %s" % (
        label, cold_ms, cold_lo, cold_hi, cold_pivots, cold_certify, "certified" if certified else "NOT certified"), flush=True)
    solver.close()
    parent.close()


def cutoff_probe(m, decimal, bounded, n_cuts):
    """One child of the table "an objective cutoff" of DESIGN.md section 10, a line per way."""
    from fractions import Fraction
    stops = hasattr(relp_amd.lib(), "relp_set_dual_cutoff")  # (a library of before the cutoff: the full re-solve alone)
    if bounded:
        import dual_bounded_lps
        case = dual_bounded_lps.BoundedCase(m, 1000 + m, n_cuts, 8, decimal=decimal, every=1)
        options = dict(certify=1, implicit_bounds=1)
        parent = relp_amd.Solver(**options).load_model(case.parent.model)
        assert parent.solve_relaxation().certified
        form, basis, _, _ = case.child(parent.basis(), parent.solution_exact())
        child, entry = form.model, "solve_dual_bounded"
    else:
        seed, _ = dual_lps.STATE_CASES[m]
        case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts, decimal=decimal)
        options = dict(certify=1)
        parent = relp_amd.Solver(**options).load_model(case.parent)
        assert parent.solve_relaxation().certified
        child, basis, _ = case.child(parent.basis(), parent.solution_exact())
        entry = "solve_dual"
    parent_optimum = Fraction(parent.objective_exact())
    parent.close()
    label = "m = %d + %d cuts, %s, %s" % (m, n_cuts, "implicit bounds" if bounded else "no bounds", "decimal" if decimal else "integer")
    solver = relp_amd.Solver(**options).load_model(child)
    optima = set()

    def full():
        started = time.perf_counter()
        result = getattr(solver, entry)(basis)
        wall = 1e3 * (time.perf_counter() - started)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        optima.add(solver.objective_exact())
        pivots = solver.dual_pivots()
        return wall, pivots, 1e3 * result.certify_seconds, 1e6 * solver.record()["dual_device_seconds"] / max(1, pivots)

    (wall, lo, hi), (pivots, _, _), (certify_ms, certify_lo, certify_hi), (device_us, us_lo, us_hi) = spread_of(full)
    assert len(optima) == 1, optima
    child_optimum = Fraction(optima.pop())
    print("%s | full %s: %.1f ms (%.1f .. %.1f), %d dual pivots, the certificate %.2f ms (%.2f .. %.2f), %.1f us (%.1f .. %.1f) of device time per dual pivot" % (
        label, entry, wall, lo, hi, pivots, certify_ms, certify_lo, certify_hi, device_us, us_lo, us_hi), flush=True)
    if stops:
        cutoff = float((parent_optimum + child_optimum) / 2)
        reasons = set()

        def stopped():
            started = time.perf_counter()
            result = getattr(solver, entry)(basis, cutoff=cutoff)
            wall = 1e3 * (time.perf_counter() - started)
            assert result.kind == relp_amd.CUTOFF and result.objective >= cutoff
            if result.certified:
                assert Fraction(cutoff) <= Fraction(solver.objective_exact()) <= child_optimum
            else:
                reasons.add(relp_amd.lib().relp_last_error(solver._h).decode())
            return wall, solver.dual_pivots(), 1e3 * result.certify_seconds, 0 if result.certified else 1

        stopped()  # warm-up
        samples = [stopped() for _ in range(RUNS)]
        (wall, lo, hi), (pivots, _, _), (certify_ms, certify_lo, certify_hi), _ = [(statistics.median(c), min(c), max(c)) for c in zip(*samples)]
        failed = sum(sample[3] for sample in samples)
        print("%s | %s under cutoff %.17g (parent %.6f, child %.6f): %.1f ms (%.1f .. %.1f), %d dual pivots, the proof %.2f ms (%.2f .. %.2f), failed in %d of %d runs%s" % (
            label, entry, cutoff, float(parent_optimum), float(child_optimum), wall, lo, hi, pivots, certify_ms, certify_lo, certify_hi, failed, RUNS,
            ": " + "; ".join(sorted(reasons)) if reasons else ""), flush=True)
        solver.set_dual_cutoff(None)
    solver.close()


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--sizes", type=int, nargs="*", default=[1025, 2049])
    parser.add_argument("--decimal", action="store_true")
    parser.add_argument("--cuts", type=int, default=0, help="cuts per child (default: those of tests/dual_lps.py)")
    parser.add_argument("--start", action="store_true", help="only the table of the dual loop's start: 4 and 24 cuts (or --cuts), integer and decimal data; "
                        "with --bounded: the starts on implicit bounds, 24 cuts (or --cuts) and a pure branch")
    parser.add_argument("--traced", action="store_true",
                        help="with --start, for a run under rocprofv3 --kernel-trace (which does not survive the replay of a captured graph: "
                             "tools/profile_r2_maxflow.sh): every handle with plain launches, and begin_dual / begin_dual_from only")
    parser.add_argument("--pricing", type=int, nargs="+", choices=[0, 1], default=None,
                        help="only the table of the leaving-row rule: the children of --start under each of the rules given")
    parser.add_argument("--bounded", action="store_true",
                        help="only the table of the loop on implicit upper bounds: a bound on every structural variable, both formulations")
    parser.add_argument("--long-step", action="store_true", help="with --bounded: implicit bounds under the plain and the long-step ratio test")
    parser.add_argument("--every", type=int, default=1, help="with --long-step: a bound on every N-th structural variable")
    parser.add_argument("--tight", type=int, default=8, help="with --long-step: tightened bounds per child")
    parser.add_argument("--farkas", action="store_true", help="only the table of the proved INFEASIBLE verdict: an infeasible child without bounds and on implicit bounds")
    parser.add_argument("--cutoff", action="store_true", help="only the table of the objective cutoff: the child re-solved to its optimum and under a "
                        "cutoff halfway to it, without bounds and on implicit bounds, integer and decimal data")
    args = parser.parse_args()
    if args.cutoff:
        for m in args.sizes:
            for bounded in (False, True):
                for decimal in ([True] if args.decimal else [False, True]):
                    cutoff_probe(m, decimal, bounded, args.cuts or 24)
        return
    if args.farkas:
        for m in args.sizes:
            for bounded in (False, True):
                farkas_probe(m, bounded)
        return
    if args.bounded and args.long_step:
        for m in args.sizes:
            for decimal in ([True] if args.decimal else [False, True]):
                long_step_probe(m, decimal, args.cuts or 24, args.tight, args.every)
        return
    if args.bounded and args.start:
        for m in args.sizes:
            for n_cuts in ([args.cuts] if args.cuts else [24, 0]):
                for decimal in ([True] if args.decimal else [False, True]):
                    bounded_start_probe(m, decimal, n_cuts, args.tight, args.traced)
        return
    if args.bounded:
        for m in args.sizes:
            for decimal in ([True] if args.decimal else [False, True]):
                bounded_probe(m, decimal, args.cuts or 24)
        return
    if args.pricing is not None:
        for m in args.sizes:
            for n_cuts in ([args.cuts] if args.cuts else [4, 24]):
                for decimal in ([True] if args.decimal else [False, True]):
                    pricing_probe(m, decimal, n_cuts, args.pricing)
        return
    if args.start:
        for m in args.sizes:
            for n_cuts in ([args.cuts] if args.cuts else [4, 24]):
                for decimal in ([True] if args.decimal else [False, True]):
                    start_probe(m, decimal, n_cuts, args.traced)
        return
    for m in args.sizes:
        probe(m, args.decimal, args.cuts)


if __name__ == "__main__":
    main()
