"""Integer LPs with a PLANTED basis for the state tests of the two LU carries (tests/test_gpu_lu_state.py, tests/test_oracle_basis_state.py).

A walk from the slack basis never produces interesting factors, so the LP comes with a basis to start from (``Solver.set_basis``), built
of blocks whose factors reach every path of the task lists of relp_amd/csrc/lu.hpp.  ``min c x, A x <= b, x >= 0``, every row with its
slack (no artificial).  The rows are partitioned into REGIONS, one per block; a region holds its block's rows, slack rows of its own
(their slacks are basic) and free columns of its own, of the lengths of ``sparse_lps.MIXES["mixed"]``, confined to the region's rows --
so no pivot ever joins two regions, and the Schur block of the exact reference (oracle/basis_state.py) stays block diagonal.  Costs are
``c = A'y + s`` with ``y <= 0``, ``s >= 0`` (dual feasible: bounded); ``b = B x0`` with ``x0 >= 1`` on every basic column, the slacks
included (primal feasible, not degenerate; asserted exactly by the tests, from the reference).  The rows are scattered by a seeded
permutation, so a block's positions lie all over [0, m).

The blocks (diagonals dominate: the planted basis has cond_2 = 6.6e3 at m = 2049, measured by tests/test_oracle_basis_state.py):

``arrow w``  w columns ``(j: 3, border: 1 | 2)`` and one with w + 1 entries ``(j: -+1, border: 3)``.  Markowitz takes the diagonal first, and
             of the last 2 x 2 the corner (equal counts: the larger entry, and the corner has grown to about 3 + w / 6): the border's row
             of L and the last column of U get w - 1 entries each (lists 0 and 2).  So the arrows are one wider than the widths below.
``fan w``    w columns ``(j: 3, hub: +-1 | 2)`` whose hub is a slack row: its slack is a column singleton and goes first, so the hub's row of U
             has w entries (list 1).  Each column is a Schur component of its own.
``chain``    a bidiagonal ``(j: a, j + 1: a)``, a = 1 .. 3, that ends on a slack row: U has one narrow slot per level, as deep as the chain is
             long.  The two entries of a column are EQUAL on purpose.  With ``(j: 3, j + 1: +-1)`` a chain that a pivot has cut is eliminated
             from the cut backwards, row singleton after row singleton, each with the multiplier 3: after 67 pivots of the f64 model at 2049
             rows ``lu_factor_host`` had max |L| = 3^23 = 9.4e10 and a last pivot of 2.8e11 on a basis of cond_2 = 1e3, and plain f64
             substitution over those factors was 7e-6 from the exact inverse (the row-relative threshold bounds the entries of a row of U
             against its pivot, not the multipliers of L).  Equal entries make every such multiplier 1.  The limit is pinned, at 1025
             rows, by ``test_known_limit_lu_factor_host_grows_l_on_a_cut_chain_of_entries_3_and_1`` (``steep_chain``, ``PLANTS["steep"]``).
``bump``     s x s, a diagonal of 9 and three +-1 per column at fixed cyclic offsets: fill, and a few levels of L.
``wide r c`` ``[D C; E F]``: r columns ``(j: 3, border row: +-1)``, c dense columns ``(every j: 1 | 2, border row: 30)``.  The 30 keeps the border
             rows out of the early pivots (threshold 0.1); the r rows of U then hold c entries each, all on ONE level.

Widths 4, 5, 9, 17, 64, 65, 256, 257 put a row into every group size G = 1 .. 64, on both sides of LU_TE G for G = 1, 16, 64, and into
the extra-entries path.  ``PLANTS``: "full" needs 1796 rows; "small" (below 2048 rows) leaves 256 and 257 out and needs 764; "tiny" is
every block kind scaled down, for the comparison with the dense reference.  "device" is for ``lu_refactor = RELP_REFACTOR_DEVICE``: the
device's elimination (lu_factor.hip) gives up on a row of the active sub-matrix beyond ``LUF_MAX_ROW = 256`` entries and the host would
factorise instead, so it is "small" plus an arrow and a fan of 180 -- rows of G = 64 in L and U, and 75 entries of room for the fill that
the 67 entered columns of moment (d) can bring (each at most one per row) -- and a chain of 500, whose INVERTED triangle has the rows
beyond 256 entries that no row of the basis, of L or of U may have there: the extra entries of the records of lu_device_tasks.hip.  (A row
of exactly 256 entries in L or U cannot be had on the device: the arrow that gives it has a border row of 258 entries in the basis.)

``task_list`` restates the slot arithmetic of ``build_tasks`` (lu.hip) and ``lu_schedules`` (lu_host.hpp) in Python; ``preconditions``
asserts from ``lu_factor_host`` of a basis what a case needs to say something.  ``HostCarry`` is the plain f64 restatement of what the
carries compute -- forward and back substitution over those rows -- behind the ``Solver`` methods that ``state_checks.assert_state`` reads,
with the three defects the planted LP is there to catch.
"""
import numpy as np

import relp_amd
from relp_amd.basis_inverse import lu_factor_host
from sparse_lps import LENGTH_CLASSES, MIXES, Provider, btrans

# relp_amd/csrc/lu.hpp and kernel_limits.hpp
LU_TE, LU_CHUNK_SLOTS, WAVE, LU_MAX_SLOTS, LU_THREADS, LU_LDS_TOTAL = 4, 1024, 64, 64, 1024, 160 * 1024 - 1024
LIST_NAMES = ("L by rows", "U by rows", "U by columns", "L by columns")  # DeviceLU::tasks[0 .. 3]
DEVICE_PIVOTS = 63 + 4  # moment (d) of the cases with the refactorisation on the device (its default period is 63)
LUF_MAX_ROW = 256  # lu_factor.hpp: the longest row of the active sub-matrix that the device's elimination takes

WIDTHS = (4, 5, 9, 17, 64, 65, 256, 257)
ARROWS = tuple(w + 1 for w in WIDTHS)  # (an arrow of width w + 1 gives rows of w entries: see ``arrow``)
PLANTS = {"full": dict(arrows=ARROWS, fans=WIDTHS, chain=200, bump=60, wide=(140, 17)),
          "small": dict(arrows=ARROWS[:6], fans=WIDTHS[:6], chain=200, bump=60, wide=(140, 17)),
          "device": dict(arrows=ARROWS[:6] + (180,), fans=WIDTHS[:6] + (180,), chain=500, bump=60, wide=(140, 17)),
          "tiny": dict(arrows=(5, 6, 10), fans=(4, 5, 9), chain=20, bump=12, wide=(12, 3))}
PLANTS["steep"] = dict(PLANTS["small"], steep=True)  # (the chain that is NOT planted: ``steep_chain``)
_cases = {}


def plant_of(m):
    return "full" if m >= 2048 else "small" if m >= 1024 else "tiny"


# ---- the blocks: (block rows, hub rows, [(own row, [(row, value)])]) in rows local to the block, the hub rows last ------------------
def _sign(rng):
    return int(rng.choice((-1, 1)))


def arrow(w, rng):
    columns = [(j, [(j, 3), (w, int(rng.randint(1, 3)))]) for j in range(w)]
    columns.append((w, [(j, 1 if rng.randint(4) == 0 else -1) for j in range(w)] + [(w, 3)]))
    return w + 1, 0, columns


def fan(w, rng):
    return w, 1, [(j, [(j, 3), (w, _sign(rng) * int(rng.randint(1, 3)))]) for j in range(w)]


def chain(length, rng):
    sizes = rng.randint(1, 4, size=length)
    return length, 1, [(j, [(j, int(sizes[j])), (j + 1, int(sizes[j]))]) for j in range(length)]


def steep_chain(length, rng):
    """The chain NOT to plant (docstring of the module): ``(j: 3, j + 1: +-1)``."""
    return length, 1, [(j, [(j, 3), (j + 1, _sign(rng))]) for j in range(length)]


def bump(s, rng):
    offsets = 1 + rng.choice(s - 1, size=3, replace=False)
    return s, 0, [(j, [(j, 9)] + [(int((j + o) % s), _sign(rng)) for o in offsets]) for j in range(s)]


def wide(r, c, rng):
    columns = [(j, [(j, 3), (r + j % c, _sign(rng))]) for j in range(r)]
    columns += [(r + k, [(j, int(rng.randint(1, 3))) for j in range(r)] + [(r + k, 30)]) for k in range(c)]
    return r + c, 0, columns


def blocks_of(plant, rng):
    spec = PLANTS[plant]
    out = [("arrow %d" % w, arrow(w, rng)) for w in spec["arrows"]] + [("fan %d" % w, fan(w, rng)) for w in spec["fans"]]
    return out + [("chain", (steep_chain if spec.get("steep") else chain)(spec["chain"], rng)), ("bump", bump(spec["bump"], rng)), ("wide", wide(*spec["wide"], rng))]


class Planted:
    """One LP: ``model``, ``provider`` (``sparse_lps.Provider``), ``basis`` (the planted basis as ``set_basis`` takes it), ``region_of_row``,
    ``region_of_column`` (provider columns, slacks included), ``region_names``, ``planted_rows`` (the rows = positions of the blocks)."""


def planted_lp(m, seed, plant=None):
    plant = plant or plant_of(m)
    rng = np.random.RandomState(seed)
    blocks = blocks_of(plant, rng)
    needed = sum(block[0] + block[1] for _, block in blocks)
    assert needed <= m, (needed, m)
    spare, scatter = m - needed, rng.permutation(m)
    columns, x0, region_of_column, basic_at = [], [], [], {}  # basic_at: row (= basis position) -> structural column
    region_of_row, slack_rows, next_row = np.zeros(m, dtype=np.int64), [], 0
    for region, (_, (n_block, n_hub, block_columns)) in enumerate(blocks):
        n_rows = n_block + n_hub + spare // len(blocks) + (region < spare % len(blocks))
        rows = scatter[next_row:next_row + n_rows]
        next_row += n_rows
        region_of_row[rows] = region
        slack_rows += rows[n_block:].tolist()
        for own, entries in block_columns:
            basic_at[int(rows[own])] = len(columns)
            columns.append(sorted((int(rows[i]), v) for i, v in entries))
            x0.append(int(rng.randint(1, 4)))
            region_of_column.append(region)
        for _ in range(n_rows):  # the region's free columns
            length = min(MIXES["mixed"][len(columns) % len(MIXES["mixed"])], n_rows)
            chosen = np.sort(rng.choice(rows, size=length, replace=False))
            values = rng.randint(1, 4, size=length) * rng.choice((-1, 1), size=length)
            columns.append([(int(i), int(v)) for i, v in zip(chosen, values)])
            x0.append(0)
            region_of_column.append(region)
    assert next_row == m
    n = len(columns)
    activity, y = np.zeros(m, dtype=np.int64), -rng.randint(0, 3, size=m)
    cost = np.zeros(n, dtype=np.int64)
    for j, column in enumerate(columns):
        for i, v in column:
            activity[i] += v * x0[j]
            cost[j] += v * y[i]
        cost[j] += int(rng.randint(0, 4))
    b = activity.copy()
    b[slack_rows] += np.maximum(0, -activity[slack_rows]) + rng.randint(1, 5, size=len(slack_rows))  # (the basic slack: >= 1)
    assert (b >= 0).all() and (cost < 0).any()
    out = Planted()
    out.model = relp_amd.Model.from_general_form(columns, ["Less"] * m, [int(v) for v in b], [(int(c), 0, None) for c in cost])
    out.provider = Provider(out.model)
    assert out.provider.m == m and not out.provider.artificial_rows
    assert [[(i, int(v)) for i, v in column] for column in out.provider.columns[:n]] == columns  # the device was given these columns
    slack_of = dict(out.provider.pivots)
    out.basis = np.array([basic_at.get(i, slack_of[i]) for i in range(m)], dtype=np.int32)
    out.region_of_row, out.region_names, out.plant, out.m, out.seed = region_of_row, [name for name, _ in blocks], plant, m, seed
    out.region_of_column = np.array(region_of_column + [0] * (out.provider.n - n), dtype=np.int64)
    for row, column in out.provider.pivots:
        out.region_of_column[column] = region_of_row[row]
    out.planted_rows = sorted(basic_at)
    return out


def case(m, seed=None, plant=None):
    """The planted LP of ``m`` rows, built once per process.  Seeds are 1000 + m, as in ``sparse_lps``."""
    key = (m, seed or 1000 + m, plant or plant_of(m))
    if key not in _cases:
        _cases[key] = planted_lp(*key)
    return _cases[key]


def basis_columns(provider, basis):
    """The columns of ``basis`` (as ``Solver.basis()``; no artificial) as ``lu_factor_host`` takes them."""
    return [[(i, float(v)) for i, v in provider.columns[int(c)]] for c in basis]


# ---- the slot arithmetic of lu.hip, restated ----------------------------------------------------------------------------------
def group_size(n):
    """G: the smallest power of two with ``LU_TE G >= n``, at most 64 (a longer row keeps the rest as extra entries)."""
    G = 1
    while G < 64 and LU_TE * G < n:
        G *= 2
    return G


def transpose(rows):
    out = [[] for _ in rows]
    for i, row in enumerate(rows):
        for j, v in row:
            out[j].append((i, v))
    return out


def four_lists(factor):
    """``[(rows, ascending)]`` of DeviceLU::tasks[0 .. 3]: row i as ``[(index it reads, value)]`` and the order the solve takes them in."""
    lower, upper = factor["lower_rows"], factor["upper_rows"]
    return [(lower, True), (upper, False), (transpose(upper), True), (transpose(lower), False)]


def task_list(rows, ascending):
    """What ``lu_schedules`` and ``build_tasks`` make of one orientation of one factor: ``lengths`` per row, ``level`` per row (0: reads
    nothing), ``chunk`` per row (-1: no entries, so no slot), ``slots`` (padding inside the chunks included, as the device counts them),
    ``chunks`` as (first, end) slot, ``level_slots`` per level, ``split_levels``: the levels that continue in a next chunk."""
    m = len(rows)
    level = [0] * m
    for i in (range(m) if ascending else range(m - 1, -1, -1)):
        level[i] = 1 + max(level[j] for j, _ in rows[i]) if rows[i] else 0
    lengths = [len(row) for row in rows]
    by_level = {}
    for i in range(m):
        if lengths[i]:
            by_level.setdefault(level[i], []).append(i)
    state = dict(slots=0, first=0)
    chunks, chunk_of, level_slots, split_levels = [], [-1] * m, {}, []

    def close_chunk():
        if state["slots"] > state["first"]:
            chunks.append((state["first"], state["slots"]))
            state["slots"] = -(-state["slots"] // WAVE) * WAVE
        state["first"] = state["slots"]
    for l in sorted(by_level):
        members = sorted(by_level[l], key=lambda i: -group_size(lengths[i]))  # (stable: widest group first)
        before = state["slots"]
        if state["slots"] - state["first"] + sum(group_size(lengths[i]) for i in members) + WAVE > LU_CHUNK_SLOTS:
            close_chunk()
            before = state["slots"]
        for i in members:
            G = group_size(lengths[i])
            if state["slots"] - state["first"] + 2 * G > LU_CHUNK_SLOTS:  # a level wider than a chunk: continue it in the next one
                close_chunk()
                split_levels.append(l)
            state["slots"] = -(-state["slots"] // G) * G + G
            chunk_of[i] = len(chunks)
        level_slots[l] = state["slots"] - before
    close_chunk()
    return dict(lengths=lengths, level=level, chunk=chunk_of, slots=chunks[-1][1] if chunks else 0, chunks=chunks, level_slots=level_slots,
                split_levels=sorted(set(split_levels)), depth=max(level) + 1, empty=sum(1 for n in lengths if n == 0))


def inverse_slots(rows):
    """``count_inverse_slots``: an inverted triangle is one level, packed widest group first without padding."""
    return sum(group_size(len(row)) for row in rows if row)


def classes(lengths):
    """The group sizes a list fills, and ">256" where a row has extra entries."""
    out = {group_size(n) for n in lengths if n}
    return sorted(out) + ([">256"] if max(lengths) > LU_TE * 64 else [])


def lds_fixed_bytes(m, max_updates, inverse_vectors=0):
    """``lu_lds_fixed_bytes`` (kernel_limits.hpp)."""
    mm = (m + 1) & ~1
    shared = ((m + 31) // 32 + 2) * 4 + ((m + 63) // 64 + 4) * 4 + 64 * 8 + 256
    if inverse_vectors:
        return inverse_vectors * mm * 8 + shared + (4 * LU_MAX_SLOTS + 2 * (LU_THREADS // 64) * LU_MAX_SLOTS) * 8
    return 2 * mm * 8 + shared + (2 * max_updates * (max_updates + 1) + 4 * LU_MAX_SLOTS) * 8


def inverse_vectors(m, max_updates):
    """``lu_inverse_vectors``: 4 LDS vectors where they fit, else 3, else 0 (the load is refused)."""
    return next((v for v in (4, 3) if lds_fixed_bytes(m, max_updates, v) <= LU_LDS_TOTAL - 2048), 0)


def last_size(inverse, max_updates, vectors=None):
    """The largest m that the carry takes with ``max_updates`` update slots (``vectors``: with that many LDS vectors, inverse form)."""
    def fits(m):
        if not inverse:
            return lds_fixed_bytes(m, max_updates) <= LU_LDS_TOTAL - 2048
        return inverse_vectors(m, max_updates) >= (vectors or 3)
    m = 1
    while fits(m + 1):
        m += 1
    return m


def class_counts(lengths):
    """``{G: rows}`` of a list, and under ">256" the rows with extra entries."""
    out = {}
    for n in lengths:
        if n:
            out[group_size(n)] = out.get(group_size(n), 0) + 1
        if n > LU_TE * 64:
            out[">256"] = out.get(">256", 0) + 1
    return out


def preconditions(columns, plant, planted=True, factorise=lu_factor_host, inverse_only=False):
    """Asserted from ``factorise`` of the basis ``columns``; returns the summary that the tests print.  Under "small" (1024 | 1025 rows)
    the widths 256 and 257 do not fit: no row of G = 64 in L by rows and U by rows, no row beyond 256 entries, no 256 | 257, in either form.
    Under "device" no row of the BASIS has more than ``LUF_MAX_ROW`` entries (asserted: the device's elimination takes it), so L and U by
    rows reach G = 64 (249 and 250 entries) but not 256 | 257 nor the extra entries; the chain gives the inverted triangles their rows
    beyond 256.  ``planted=False``: a basis some pivots away from the planted one -- a pivot may have taken a column out of any block, so
    only what no single block carries is asserted: the lists of more than one chunk and, under "full" and "device", a row beyond 256
    entries.  ``factorise``: ``lu_factor_host``, or ``lu_factor_device`` with the dense tail the solver uses -- the rows the DEVICE made,
    with pivots of its own; ``inverse_only``: nothing is asserted on the four lists of the Forrest-Tomlin form (the device builds the
    inverse-factor form only)."""
    full, device = plant == "full", plant == "device"
    factor, inverted = factorise(columns), factorise(columns, inverted=True)
    lists = [task_list(rows, ascending) for rows, ascending in four_lists(factor)]
    summary = {}
    for name, info in zip(LIST_NAMES, lists):
        summary[name] = dict(slots=info["slots"], chunks=len(info["chunks"]), depth=info["depth"], classes=class_counts(info["lengths"]),
                             widest_level=max(info["level_slots"].values()), split_levels=info["split_levels"], empty=info["empty"])
        assert info["empty"] > 0 and info["empty"] < len(info["lengths"]), name  # a row without entries and one with
    inverse = [inverted["lower_rows"], inverted["upper_rows"], transpose(inverted["upper_rows"]), transpose(inverted["lower_rows"])]
    summary["inverse slots"] = [inverse_slots(rows) for rows in inverse]
    summary["inverse longest row"] = [max(len(row) for row in rows) for rows in inverse]
    summary["inverse classes"] = [class_counts([len(row) for row in rows]) for rows in inverse]
    summary["inverse extra entries"] = [sum(max(0, len(row) - LU_TE * 64) for row in rows) for rows in inverse]
    row_of_basis = np.zeros(len(columns), dtype=np.int64)
    for column in columns:
        for i, _ in column:
            row_of_basis[i] += 1
    summary["longest row of the basis"] = int(row_of_basis.max())
    if device:  # (planted: room for the fill of DEVICE_PIVOTS entered columns, each at most one more entry in a row of the active sub-matrix)
        assert summary["longest row of the basis"] <= LUF_MAX_ROW - (DEVICE_PIVOTS + 1 if planted else 0)
    assert sum(1 for slots in summary["inverse slots"] if slots > LU_CHUNK_SLOTS) >= 2
    if full or device:
        assert max(summary["inverse longest row"]) > LU_TE * 64 and max(summary["inverse extra entries"]) > 0
    if not inverse_only:
        assert sum(1 for info in lists if info["slots"] > LU_CHUNK_SLOTS) >= 2
        if full and not planted:
            assert max(max(info["lengths"]) for info in lists) > LU_TE * 64
    if not planted:
        return summary
    # the inverted triangles: every group size in the rows of L^-1 and U^-1 together (the arrows, the fans and the chain; where the
    # device's pivots put a block into the other triangle it is still among these two)
    groups = {1, 2, 4, 8, 16, 32, 64} if full or device else {1, 2, 4, 8, 16, 32}
    assert set(summary["inverse classes"][0]) | set(summary["inverse classes"][1]) >= groups
    assert (max(summary["inverse longest row"]) > LU_TE * 64) == (full or device)
    if inverse_only:
        return summary
    for info, name in zip(lists[:2], LIST_NAMES):
        lengths = set(info["lengths"])
        assert {group_size(n) for n in lengths if n} >= groups, name
        assert lengths >= ({4, 5, 64, 65, 256, 257} if full else {4, 5, 64, 65}), name  # both sides of LU_TE G for G = 1, 16 (and 64)
        assert (max(lengths) > LU_TE * 64) == full, name
    # the column orientations: U by columns has the arrows' last columns (every class) and the wide block's dense columns; L by columns
    # cannot get a class beyond G = 4 from any of the blocks -- Markowitz takes column singletons first, so a long column always lands in
    # U; it gets its columns of up to 16 entries from the bump and the wide block
    assert set(classes(lists[2]["lengths"])) >= set(classes(lists[0]["lengths"]))
    assert set(classes(lists[3]["lengths"])) >= {1, 2, 4}
    assert any(len(info["chunks"]) > 1 for info in lists)
    assert max(lists[1]["level_slots"].values()) > LU_CHUNK_SLOTS and lists[1]["split_levels"]  # one level wider than a chunk
    assert max(info["depth"] for info in lists) >= 100
    return summary


# ---- what to check ---------------------------------------------------------------------------------------------------------------
def checks_of(lp, exact):
    """The arguments of ``assert_state``: every row of the inverse up to 4400 rows -- beyond, every row that may not be a unit vector (all
    positions of the blocks are among them), rows 0 and m - 1, both sides of every multiple of 512 and every 16th --; the three full
    BTRANs; one free column per region and length class, and the columns with the most and the fewest non-zeros in alpha."""
    m = exact.m
    rows = range(m)
    if m > 4400:
        chosen = set(exact.rows_that_may_not_be_unit().tolist()) | {0, m - 1} | set(range(0, m, 16))
        for edge in range(512, m, 512):
            chosen |= {edge - 1, edge}
        rows = sorted(chosen)
    free = np.flatnonzero(~exact.is_basic)
    lengths = np.array([lp.provider.length_of(int(j)) for j in free])
    columns = set()
    for region in range(len(lp.region_names)):
        for low, high in LENGTH_CLASSES:
            found = np.flatnonzero((lp.region_of_column[free] == region) & (lengths >= low) & (lengths <= high))
            if len(found):
                columns.add(int(free[found[0]]))
    estimates = exact.alpha_nnz_estimates(free)
    columns |= {int(free[np.argmax(estimates)]), int(free[np.argmin(estimates)])}
    return dict(inverse_rows=rows, alpha_columns=sorted(columns), btrans=btrans(m))


# ---- the f64 restatement ------------------------------------------------------------------------------------------------------------
DEFECTS = ("entries beyond LU_TE 64 dropped", "last slot of a G = 64 group dropped", "second chunk skipped")


class HostCarry:
    """The state of ``basis`` as plain f64 forward and back substitution over the rows of ``lu_factor_host`` gives it, behind the methods of
    ``Solver`` that ``assert_state`` reads.  ``defect``: one of ``DEFECTS`` -- what a wrong kernel would do to a task list: drop the extra
    entries of a row (beyond the first ``LU_TE * 64``), drop what slot 63 of a 64-slot group holds (entries 63, 127, 191, 255: slot j takes
    j, j + G, ...), or never solve the rows whose slots lie in the second chunk."""

    def __init__(self, provider, basis, defect=None):
        assert defect is None or defect in DEFECTS
        self.m, self.n, self.n_art = provider.m, provider.n, 0
        m = self.m
        factor = lu_factor_host(basis_columns(provider, basis))
        self.rowpos, self.colpos, self.diag = np.array(factor["rowpos"]), np.array(factor["colpos"]), np.array(factor["diag"])
        self.lists = []
        for rows, ascending in four_lists(factor):
            info = task_list(rows, ascending)
            kept = []
            for i, row in enumerate(rows):
                if defect == DEFECTS[0]:
                    row = row[:LU_TE * 64]
                elif defect == DEFECTS[1] and group_size(len(row)) == 64:
                    row = [entry for e, entry in enumerate(row) if e >= LU_TE * 64 or e % 64 != 63]
                skipped = defect == DEFECTS[2] and info["chunk"][i] == 1
                kept.append(None if skipped else (np.array([j for j, _ in row], dtype=np.int64), np.array([v for _, v in row])))
            self.lists.append((kept, ascending))
        self.basis = np.array(basis, dtype=np.int64)
        self.A = np.zeros((m, self.n))
        for j, column in enumerate(provider.columns):
            for i, v in column:
                self.A[i, j] = float(v)
        self.cost = np.array([float(c) for c in provider.cost] + [0.0] * (self.n - len(provider.cost)))
        self.rhs = np.array([float(v) for v in provider.b])
        self.free = np.setdiff1d(np.arange(self.n), self.basis)
        self._priced = None

    def _solve(self, which, X, diag):
        kept, ascending = self.lists[which]
        for i in (range(self.m) if ascending else range(self.m - 1, -1, -1)):
            if kept[i] is None:
                continue
            where, values = kept[i]
            if len(where):
                X[i] -= values @ X[where]
            if diag:
                X[i] /= self.diag[i]
        return X

    def ftran(self, Y):
        """``B^-1 Y`` for the columns of ``Y``."""
        X = np.zeros(Y.shape)
        X[self.rowpos] = Y
        return self._solve(1, self._solve(0, X, False), True)[self.colpos]

    def btran(self, W):
        """``(w' B^-1)'`` for the columns ``w`` of ``W``."""
        X = np.zeros(W.shape)
        X[self.colpos] = W
        return self._solve(3, self._solve(2, X, True), False)[self.rowpos]

    def _price(self):
        if self._priced is None:
            pi = self.btran(self.cost[self.basis][:, None])[:, 0]
            costs = self.cost - pi @ self.A
            gamma = np.full(self.n, np.nan)
            self.alphas = self.ftran(self.A[:, self.free])
            gamma[self.free] = 1.0 + (self.alphas * self.alphas).sum(axis=0)
            self._priced = costs, gamma
        return self._priced

    def select_primal_pivot_column(self):
        costs, gamma = self._price()
        key = np.where(costs[self.free] < -1e-9, costs[self.free] ** 2 / gamma[self.free], -1.0)
        return (int(self.free[np.argmax(key)]), float(costs[self.free[np.argmax(key)]])) if key.max() > 0 else None

    def relative_costs(self):
        return self._price()[0]

    def gamma(self):
        return self._price()[1]

    def select_primal_pivot_row(self, q):
        self._price()
        return None, self.alphas[:, int(np.flatnonzero(self.free == q)[0])]

    def basis_inverse_row(self, i):
        if not hasattr(self, "inverse"):
            self.inverse = self.btran(np.eye(self.m)).T.copy()
        return self.inverse[i]

    def right_multiply_by_basis_inverse(self, rows, values):
        w = np.zeros((self.m, 1))
        np.add.at(w[:, 0], rows, values)
        return self.btran(w)[:, 0]

    def b(self):
        return self.ftran(self.rhs[:, None])[:, 0]

    def objective_function_value(self):
        return float(self.cost[self.basis] @ self.b())
