"""The f64 state of a handle on the two LU carries -- RELP_CARRY_LU (Forrest-Tomlin) and RELP_CARRY_LU_INVERSE (inverse factors, product form)
-- against the exact state of its basis, from a PLANTED basis whose factors reach every path of the task lists (``-m gpu``, a real MI355X).

The LPs are those of tests/lu_lps.py: blocks that put a row of L, U, L^-1 and U^-1 into every group size G = 1 .. 64, on both sides of
LU_TE G, into the extra entries beyond 256, more than one chunk of 1024 slots into the lists, one level wider than a chunk, a chain 200 levels
deep -- asserted on the CPU (tests/test_oracle_basis_state.py) and again here, from ``lu_factor_host`` of the basis the device ends on (there
without the exact row lengths: a pivot may take a column of a block out).  Every case: ``Solver(carry, refactor_period, polish_period=0,
certify=0)``, the plan fields that name it, ``set_basis(planted)`` -- a factorisation and an upload, phase two --, its MOMENT, then
``assert_state`` (tests/state_checks.py, tolerances of an un-polished state, unchanged) against ``SparseBasisState`` of ``solver.basis()``:
rows of the inverse (all up to 4400 rows; beyond, every row that may not be a unit vector, rows 0 and m - 1, both sides of every multiple of
512 and every 16th), x_B, the objective, every relative cost, every steepest-edge weight, three BTRANs with a non-zero in every row, FTRANs
through ``select_primal_pivot_row`` (one free column per region and length class, the longest and the shortest alpha) and the entering choice.

Moments: (a) straight after ``set_basis`` -- the fresh factors alone; (b) one pivot -- the first spike, eta, kept column; (c) ``refactor_period``
pivots in one ``iterate`` -- every update slot used; (d) ``refactor_period + 4`` pivots -- across one refactorisation of a basis that holds
entered columns.  Sizes (kernel_limits.hpp; ``lu_lps.lds_fixed_bytes`` restates ``lu_lds_fixed_bytes``, anchored on the CPU against the plan):
1024 | 1025 (a thread's second row; the plant without the widths 256 and 257 -- no row of G = 64 in L and U by rows, none beyond 256
entries), 2048 | 2049, 4396 | 4397 (the inverse-factor form goes from four LDS vectors to three), 5850 and 8712 (the last sizes the two
carries take at their default periods).  All four moments and the periods 7, default and 63 at 2049; (a) and (c) elsewhere.
``lu_refactor = RELP_REFACTOR_DEVICE`` (lu_factor.hip, lu_device_tasks.hip: the second builder of the lists) at 2049 and 4397, (a) and (d),
on a plant of its own (``lu_lps.PLANTS["device"]``): the device's elimination gives up on a row of more than 256 entries and the host
would factorise instead, so the widest arrow and fan are 180 (G = 64 in L and U, no extra entries there) and a chain of 500 gives the
inverted triangles their rows beyond 256.  There the preconditions are asserted twice: from ``lu_factor_host`` and from the rows the DEVICE
makes of the basis it ends on (``lu_factor_device``, the solver's dense tail of 8) -- its pivots are its own, and they halve the chain
again and again instead of following it, so its inverted triangles are far smaller than the host's (3482 against 29424 slots in U^-1 by
rows at 2049) and hold 1 to 21 rows beyond 256 entries, in L^-1 by rows and in U^-1 by columns: printed per case, below.

The reference: 1.5 s for the planted basis of 2049 rows (k = 1787 non-unit columns in 688 components, the largest 259; 26 s before the
Schur block was inverted by components); a walked basis re-uses the components no pivot touched.  Exact states are kept per basis.

Largest error per part (as in tests/test_gpu_sparse_state.py), the f64 restatement on the CPU (``lu_lps.HostCarry``, planted basis, 2049 rows)
first -- it must stay within 1 / 100 of the tolerance, asserted in tests/test_oracle_basis_state.py --, then the device, one line per case:

  restatement 2049                 inverse 2.8e-15  x_B 2.9e-15  objective 0.0e+00  costs 2.8e-13  weights 1.8e-14  alpha 5.1e-16  btran 5.6e-16
  lu 1024 period 31 (a)            inverse 1.3e-15  x_B 2.5e-16  objective 0.0e+00  costs 1.4e-13  weights 1.2e-15  alpha 3.4e-16  btran 8.2e-16  (0 entered, 1.1 s)
  lu 1024 period 31 (c)            inverse 1.1e-14  x_B 3.3e-16  objective 5.8e-16  costs 1.8e-12  weights 2.1e-12  alpha 4.0e-15  btran 1.4e-14  (26 entered, 0.6 s)
  lu 1025 period 31 (a)            inverse 1.1e-15  x_B 1.5e-15  objective 0.0e+00  costs 1.8e-13  weights 1.1e-15  alpha 4.4e-16  btran 9.5e-16  (0 entered, 0.8 s)
  lu 1025 period 31 (c)            inverse 2.0e-15  x_B 1.5e-15  objective 1.6e-16  costs 3.7e-13  weights 1.2e-13  alpha 1.9e-15  btran 1.1e-15  (31 entered, 0.7 s)
  lu 2048 period 31 (a)            inverse 2.1e-15  x_B 8.9e-16  objective 0.0e+00  costs 3.4e-13  weights 1.6e-15  alpha 2.1e-15  btran 1.8e-15  (0 entered, 2.3 s)
  lu 2048 period 31 (c)            inverse 3.1e-15  x_B 8.9e-16  objective 2.1e-16  costs 3.4e-13  weights 1.1e-12  alpha 2.1e-15  btran 1.1e-15  (27 entered, 2.1 s)
  lu_inverse 1024 period 47 (a)    inverse 1.3e-15  x_B 1.0e-15  objective 0.0e+00  costs 2.1e-13  weights 4.4e-16  alpha 2.6e-16  btran 4.0e-16  (0 entered, 0.3 s)
  lu_inverse 1024 period 47 (c)    inverse 2.1e-14  x_B 1.1e-14  objective 0.0e+00  costs 3.1e-13  weights 1.3e-13  alpha 1.2e-14  btran 1.2e-14  (40 entered, 0.6 s)
  lu_inverse 1025 period 47 (a)    inverse 2.9e-15  x_B 3.6e-15  objective 1.7e-16  costs 2.2e-13  weights 4.9e-16  alpha 1.2e-15  btran 9.3e-16  (0 entered, 0.3 s)
  lu_inverse 1025 period 47 (c)    inverse 2.5e-14  x_B 3.6e-15  objective 1.6e-16  costs 6.2e-13  weights 3.8e-13  alpha 4.2e-15  btran 6.9e-15  (45 entered, 0.7 s)
  lu_inverse 2048 period 47 (a)    inverse 3.2e-15  x_B 1.4e-15  objective 0.0e+00  costs 3.2e-13  weights 6.1e-16  alpha 1.5e-15  btran 1.1e-15  (0 entered, 1.1 s)
  lu_inverse 2048 period 47 (c)    inverse 3.2e-15  x_B 1.4e-15  objective 6.4e-16  costs 2.4e-13  weights 1.3e-13  alpha 2.3e-15  btran 9.7e-16  (43 entered, 2.0 s)
  lu 2049 period 31 (a)            inverse 2.7e-15  x_B 2.1e-15  objective 0.0e+00  costs 2.2e-13  weights 1.2e-15  alpha 3.9e-16  btran 9.0e-16  (0 entered, 2.4 s)
  lu 2049 period 31 (b)            inverse 2.7e-15  x_B 2.1e-15  objective 0.0e+00  costs 2.0e-13  weights 1.2e-15  alpha 3.9e-16  btran 9.0e-16  (1 entered, 1.9 s)
  lu 2049 period 31 (c)            inverse 2.7e-15  x_B 2.1e-15  objective 0.0e+00  costs 2.0e-13  weights 1.7e-14  alpha 1.6e-15  btran 1.2e-15  (30 entered, 2.2 s)
  lu 2049 period 31 (d)            inverse 1.0e-15  x_B 1.5e-15  objective 1.1e-16  costs 5.4e-13  weights 1.6e-14  alpha 6.0e-16  btran 7.0e-16  (34 entered, 2.0 s)
  lu 2049 period 7 (a)             inverse 2.7e-15  x_B 2.1e-15  objective 0.0e+00  costs 2.2e-13  weights 1.2e-15  alpha 3.9e-16  btran 9.0e-16  (0 entered, 1.3 s)
  lu 2049 period 7 (b)             inverse 2.7e-15  x_B 2.1e-15  objective 0.0e+00  costs 2.0e-13  weights 1.2e-15  alpha 3.9e-16  btran 9.0e-16  (1 entered, 1.2 s)
  lu 2049 period 7 (c)             inverse 2.7e-15  x_B 2.1e-15  objective 0.0e+00  costs 1.6e-13  weights 8.7e-15  alpha 5.1e-16  btran 9.0e-16  (7 entered, 1.9 s)
  lu 2049 period 7 (d)             inverse 1.9e-15  x_B 4.0e-16  objective 0.0e+00  costs 2.1e-13  weights 1.5e-14  alpha 4.0e-16  btran 9.0e-16  (11 entered, 2.0 s)
  lu 2049 period 63 (a)            inverse 2.7e-15  x_B 2.1e-15  objective 0.0e+00  costs 2.2e-13  weights 1.2e-15  alpha 3.9e-16  btran 9.0e-16  (0 entered, 1.2 s)
  lu 2049 period 63 (b)            inverse 2.7e-15  x_B 2.1e-15  objective 0.0e+00  costs 2.0e-13  weights 1.2e-15  alpha 3.9e-16  btran 9.0e-16  (1 entered, 1.3 s)
  lu 2049 period 63 (c)            inverse 5.0e-15  x_B 2.6e-15  objective 1.1e-16  costs 1.0e-12  weights 9.7e-13  alpha 3.2e-15  btran 1.6e-15  (61 entered, 2.0 s)
  lu 2049 period 63 (d)            inverse 1.3e-15  x_B 1.3e-15  objective 0.0e+00  costs 5.4e-13  weights 9.7e-13  alpha 7.6e-16  btran 4.7e-16  (65 entered, 1.9 s)
  lu_inverse 2049 period 47 (a)    inverse 5.5e-15  x_B 1.7e-15  objective 0.0e+00  costs 2.4e-13  weights 4.9e-16  alpha 3.8e-16  btran 3.3e-15  (0 entered, 1.1 s)
  lu_inverse 2049 period 47 (b)    inverse 5.5e-15  x_B 1.7e-15  objective 0.0e+00  costs 2.1e-13  weights 4.9e-16  alpha 3.8e-16  btran 1.9e-15  (1 entered, 1.1 s)
  lu_inverse 2049 period 47 (c)    inverse 1.3e-14  x_B 1.8e-15  objective 2.3e-16  costs 2.7e-13  weights 9.6e-14  alpha 9.4e-15  btran 2.4e-15  (45 entered, 2.0 s)
  lu_inverse 2049 period 47 (d)    inverse 1.8e-15  x_B 1.6e-14  objective 1.1e-16  costs 5.4e-13  weights 9.7e-14  alpha 1.0e-15  btran 6.7e-16  (49 entered, 1.7 s)
  lu_inverse 2049 period 7 (a)     inverse 5.5e-15  x_B 1.7e-15  objective 0.0e+00  costs 2.4e-13  weights 4.9e-16  alpha 3.8e-16  btran 3.3e-15  (0 entered, 1.2 s)
  lu_inverse 2049 period 7 (b)     inverse 5.5e-15  x_B 1.7e-15  objective 0.0e+00  costs 2.1e-13  weights 4.9e-16  alpha 3.8e-16  btran 1.9e-15  (1 entered, 1.1 s)
  lu_inverse 2049 period 7 (c)     inverse 5.5e-15  x_B 1.7e-15  objective 0.0e+00  costs 1.8e-13  weights 1.0e-14  alpha 3.8e-16  btran 4.8e-16  (7 entered, 1.1 s)
  lu_inverse 2049 period 7 (d)     inverse 9.9e-16  x_B 1.4e-15  objective 1.1e-16  costs 2.7e-13  weights 8.4e-15  alpha 6.3e-16  btran 1.5e-15  (11 entered, 1.1 s)
  lu_inverse 2049 period 63 (a)    inverse 5.5e-15  x_B 1.7e-15  objective 0.0e+00  costs 2.4e-13  weights 4.9e-16  alpha 3.8e-16  btran 3.3e-15  (0 entered, 1.2 s)
  lu_inverse 2049 period 63 (b)    inverse 5.5e-15  x_B 1.7e-15  objective 0.0e+00  costs 2.1e-13  weights 4.9e-16  alpha 3.8e-16  btran 1.9e-15  (1 entered, 1.1 s)
  lu_inverse 2049 period 63 (c)    inverse 1.3e-14  x_B 2.4e-15  objective 0.0e+00  costs 3.0e-13  weights 9.7e-14  alpha 9.3e-15  btran 2.5e-15  (61 entered, 1.2 s)
  lu_inverse 2049 period 63 (d)    inverse 1.8e-15  x_B 1.9e-14  objective 2.2e-16  costs 5.4e-13  weights 9.7e-14  alpha 1.0e-15  btran 6.7e-16  (65 entered, 1.3 s)
  lu_inverse 4396 period 47 (a)    inverse 6.1e-15  x_B 6.0e-15  objective 0.0e+00  costs 2.2e-12  weights 4.5e-16  alpha 7.1e-16  btran 6.6e-15  (0 entered, 3.7 s)
  lu_inverse 4396 period 47 (c)    inverse 9.9e-15  x_B 6.0e-15  objective 1.1e-16  costs 2.2e-12  weights 1.4e-13  alpha 1.7e-15  btran 1.2e-15  (43 entered, 3.4 s)
  lu_inverse 4397 period 47 (a)    inverse 3.3e-14  x_B 9.0e-15  objective 1.1e-15  costs 5.7e-12  weights 4.1e-16  alpha 8.7e-16  btran 9.2e-15  (0 entered, 3.5 s)
  lu_inverse 4397 period 47 (c)    inverse 3.3e-14  x_B 1.0e-14  objective 9.5e-16  costs 5.7e-12  weights 1.3e-12  alpha 4.9e-15  btran 4.9e-15  (41 entered, 3.3 s)
  lu_inverse 5850 period 47 (a)    inverse 4.4e-16  x_B 4.7e-15  objective 0.0e+00  costs 4.6e-13  weights 4.6e-16  alpha 2.0e-16  btran 6.8e-16  (0 entered, 3.4 s)
  lu_inverse 5850 period 47 (c)    inverse 2.5e-15  x_B 4.5e-15  objective 8.6e-16  costs 3.8e-13  weights 1.8e-13  alpha 6.2e-16  btran 1.3e-15  (44 entered, 3.5 s)
  lu 4397 period 31 (a)            inverse 1.1e-14  x_B 1.3e-15  objective 2.4e-16  costs 1.5e-12  weights 9.6e-16  alpha 6.7e-16  btran 8.1e-15  (0 entered, 2.2 s)
  lu 4397 period 31 (c)            inverse 1.1e-14  x_B 1.3e-15  objective 3.6e-16  costs 1.5e-12  weights 7.1e-13  alpha 1.2e-14  btran 1.9e-15  (27 entered, 3.7 s)
  lu 8712 period 31 (a)            inverse 1.6e-15  x_B 4.2e-16  objective 0.0e+00  costs 3.6e-13  weights 8.9e-16  alpha 1.5e-16  btran 7.4e-16  (0 entered, 4.9 s)
  lu 8712 period 31 (c)            inverse 2.3e-15  x_B 4.2e-16  objective 4.2e-16  costs 6.4e-13  weights 1.0e-12  alpha 1.0e-15  btran 1.4e-15  (31 entered, 4.0 s)
  lu_inverse 2049 device refactorisation (a) inverse 7.4e-16  x_B 1.0e-15  objective 0.0e+00  costs 3.3e-13  weights 4.3e-16  alpha 2.0e-16  btran 2.8e-16  (0 entered, 3.3 s)
  lu_inverse 2049 device refactorisation (d) inverse 3.7e-15  x_B 5.1e-15  objective 0.0e+00  costs 5.7e-13  weights 6.6e-13  alpha 1.5e-15  btran 1.2e-15  (63 entered, 1.9 s)
  lu_inverse 4397 device refactorisation (a) inverse 4.7e-15  x_B 6.0e-15  objective 0.0e+00  costs 8.7e-13  weights 4.0e-16  alpha 1.8e-15  btran 8.3e-16  (0 entered, 4.4 s)
  lu_inverse 4397 device refactorisation (d) inverse 8.0e-15  x_B 1.1e-13  objective 1.1e-16  costs 7.3e-13  weights 3.7e-13  alpha 3.4e-15  btran 2.3e-15  (63 entered, 2.9 s)
  lu 2049 period 31 (d), plain launches inverse 1.0e-15  x_B 1.5e-15  objective 1.1e-16  costs 5.4e-13  weights 1.6e-14  alpha 6.0e-16  btran 7.0e-16  (34 entered, 1.2 s)
  lu 2049 seed 4049 period 31 (c), stepped, 2 positions twice inverse 3.1e-15  x_B 5.2e-16  objective 0.0e+00  costs 3.2e-13  weights 1.0e-13  alpha 4.5e-15  btran 3.4e-15  (29 entered, 2.3 s)
  lu 2049 seed 4049 period 31 (c), the same walk in one batch inverse 3.1e-15  x_B 5.2e-16  objective 0.0e+00  costs 3.2e-13  weights 1.0e-13  alpha 4.5e-15  btran 3.4e-15  (29 entered, 3.5 s)

(seconds: the whole case with its reference; a case whose basis an earlier case ended on re-uses that reference.)  Slots of the four lists
(L by rows, U by rows, U by columns, L by columns) at the planted basis: 1024: 296 / 1760 / 2488 / 462, 1025: 296 / 1783 / 2541 / 479,
2048: 456 / 2480 / 3055 / 996, 2049: 432 / 2428 / 3118 / 992, 4397: 424 / 2425 / 3214 / 988, 8712: 440 / 2468 / 3085 / 1040; of the four
inverted triangles at 2049: 1161 / 10727 / 10970 / 1449 (up to eleven rounds of slots per thread), at 5850: 1083 / 14402 / 14672 / 1342;
the four lists again at 4396: 440 / 2385 / 3133 / 1059, at 5850: 400 / 2401 / 3065 / 968; chunks 1 / 3 / 3 / 1 at 1024 | 1025, 1 / 4 / 4 / 2 from 2048 on.

Rows per group size (G: rows; ">256": rows with extra entries) of the four lists at the planted basis:
  1024  L by rows 1:21 2:13 4:12 8:17 16:1 32:1 | U by rows 1:404 2:30 4:14 8:141 16:1 32:1 | U by columns 1:390 2:5 4:6 8:8 16:1 32:1 64:17 | L by columns 1:344 2:27 4:14
  1025  L by rows 1:22 2:9 4:15 8:17 16:1 32:1 | U by rows 1:406 2:20 4:22 8:141 16:1 32:1 | U by columns 1:388 2:4 4:9 8:9 16:1 32:1 64:17 | L by columns 1:342 2:24 4:19
  2048  L by rows 1:29 2:5 4:12 8:21 16:1 32:1 64:2 >256:1 | U by rows 1:917 2:23 4:23 8:141 16:1 32:1 64:2 >256:1 | U by columns 1:899 2:8 4:8 8:9 16:1 32:1 64:19 >256:1 | L by columns 1:861 2:18 4:21
  2049  L by rows 1:26 2:5 4:16 8:17 16:1 32:1 64:2 >256:1 | U by rows 1:921 2:22 4:20 8:141 16:1 32:1 64:2 >256:1 | U by columns 1:901 2:7 4:7 8:9 16:1 32:1 64:19 >256:1 | L by columns 1:863 2:18 4:19
  4396  L by rows 1:27 2:3 4:17 8:18 16:1 32:1 64:2 >256:1 | U by rows 1:920 2:23 4:20 8:141 16:1 32:1 64:2 >256:1 | U by columns 1:902 2:3 4:8 8:10 16:1 32:1 64:19 >256:1 | L by columns 1:861 2:17 4:22
  4397  L by rows 1:23 2:7 4:18 8:15 16:1 32:1 64:2 >256:1 | U by rows 1:925 2:20 4:18 8:141 16:1 32:1 64:2 >256:1 | U by columns 1:904 2:7 4:9 8:7 16:1 32:1 64:19 >256:1 | L by columns 1:865 2:18 4:17
  5850  L by rows 1:21 2:8 4:23 8:10 16:1 32:1 64:2 >256:1 | U by rows 1:927 2:27 4:8 8:141 16:1 32:1 64:2 >256:1 | U by columns 1:900 2:8 4:15 8:1 16:1 32:1 64:19 >256:1 | L by columns 1:865 2:24 4:10
  8712  L by rows 1:23 2:10 4:12 8:18 16:1 32:1 64:2 >256:1 | U by rows 1:923 2:19 4:21 8:141 16:1 32:1 64:2 >256:1 | U by columns 1:903 2:6 4:9 8:8 16:1 32:1 64:19 >256:1 | L by columns 1:857 2:22 4:21
(L by columns cannot go beyond G = 4: Markowitz takes column singletons first, so a long column always lands in U.)  The inverted triangles
(L^-1 by rows, U^-1 by rows, U^-1 by columns, L^-1 by columns) at 2049: 1:13 2:6 4:8 8:6 16:18 32:10 64:7 >256:3 | 1:1635 2:14 4:44 8:183
16:32 32:66 64:75 >256:2 | 1:1794 2:12 4:14 8:21 16:46 32:68 64:94 >256:4 | 1:727 2:41 4:104 8:28.  The plant of the device cases at 2049,
from the host's rows: lists 320 / 2254 / 2918 / 628 slots, inverted 914 / 29424 / 29617 / 955 with 245 rows beyond 256 in U^-1; from the
DEVICE's own rows, (a): inverted 1620 / 3482 / 3836 / 1905 slots, longest rows 354 / 40 / 255 / 16, L^-1 by rows 1:178 2:39 4:19 8:31 16:11
32:11 64:8 >256:1; (d): 1985 / 4600 / 4628 / 2337 slots, longest 283 / 40 / 471 / 31, 2 rows beyond 256 in L^-1 by rows and 7 in U^-1 by
columns (1088 extra entries).  At 4397, (a): 1670 / 5999 / 6321 / 1922, longest 263 / 129 / 258 / 22; (d): 1997 / 7200 / 7077 / 2203, longest
263 / 133 / 310 / 68, 21 rows beyond 256 in U^-1 by columns (778 extra entries).

What the cases found: ``set_basis`` on a freshly loaded handle with ``lu_refactor = RELP_REFACTOR_DEVICE`` threw "refactor_device before
prepare_device" -- only ``begin_phase_one`` sized the arrays the refactorisation kernels write into; ``invert_from_scratch`` does it now
where it has not been done.  And on the way here, on the CPU: a bidiagonal chain with entries 3 and 1, once a pivot has cut it, makes
``lu_factor_host`` eliminate it backwards with the multiplier 3 each time -- max |L| = 3^23 on a basis of cond_2 = 1e3, 7e-6 lost in
plain f64 substitution (docstring of tests/lu_lps.py).  The row-relative threshold does not bound the multipliers of L; the planted chain
has equal entries so that the cases measure the kernels and not this; tests/test_oracle_basis_state.py pins the limit.  And the device's
elimination falls back to the host where fill takes a row of the active sub-matrix past 256 entries: with an arrow and a fan of 250 the
planted basis went through, the basis 67 pivots on did not (``device_refactor_fallbacks`` = 1), hence the 180.  No kernel was found wrong:
every part of every case is within 1.2e-13 (1e-11 for the costs and 3e-12 for the weights) of the exact state.

Open: ``implicit_bounds = 1`` with the LU carries (the reference has no bounded state yet) and the refactorisation beside the pivots
(``RELP_REFACTOR_DEVICE_ASYNC``) are not covered here.
"""
import time

import numpy as np
import pytest

import relp_amd
from relp_amd.api import CARRY_LU, CARRY_LU_INVERSE
from relp_amd.basis_inverse import lu_factor_device
from state_checks import assert_state
import lu_lps

pytestmark = pytest.mark.gpu
REFACTOR_DEVICE = 1
NAMES = {CARRY_LU: "lu", CARRY_LU_INVERSE: "lu_inverse"}
DENSE_TAIL = 8  # Solver::refactor_lu_device: the dense tail of the device's elimination unless an option says otherwise
_states = {}


def exact_state(lp, basis):
    """``(exact state, what to check)`` of a basis.  Kept for ONE LP at a time, and of it the planted basis and the last other one: the
    cases of one size follow each other, start from the same basis and often end on the one the case before ended on.  (A state of the
    full plant holds a dense 1787 x 1787 longdouble block: 50 MB.)"""
    lp_key = (lp.m, lp.seed, lp.plant)
    key = lp_key + (tuple(int(c) for c in basis),)
    if key not in _states:
        planted = lp_key + (tuple(int(c) for c in lp.basis),)
        for other in list(_states):
            if other[:3] != lp_key or other != planted:
                del _states[other]
        exact = lp.provider.state(basis, 2)
        _states[key] = exact, lu_lps.checks_of(lp, exact)
    return _states[key]


def device_factorisation(columns, inverted=False):
    """The rows that lu_factor.hip and the inversion kernels of lu_device_tasks.hip make of a basis, with the solver's dense tail."""
    return lu_factor_device(columns, inverted=inverted, dense_tail=DENSE_TAIL)


def period_of(carry, period, device):
    return period or (63 if device else 47 if carry == CARRY_LU_INVERSE else 31)


def pivots_of(moment, period):
    return {"a": 0, "b": 1, "c": period, "d": period + 1 + 3}[moment]


def prepared(carry, m, period=0, device=False, plant=None, seed=None, **options):
    """A handle at the planted basis of the LP, the plan fields asserted; returns (solver, lp, refactor period)."""
    lp = lu_lps.case(m, seed=seed, plant=plant)
    options = dict(carry=carry, refactor_period=period, polish_period=0, certify=0, **options)
    if device:
        options["lu_refactor"] = REFACTOR_DEVICE
    plan = lp.model.kernel_path(**options)
    expected = dict(lu_mode=True, lu_inverse=carry == CARRY_LU_INVERSE, refactor_period=period_of(carry, period, device), device_refactor=device, n_art=0)
    for field, value in expected.items():
        assert plan[field] == value, (field, plan[field], value)
    solver = relp_amd.Solver(**options).load_model(lp.model)
    try:
        solver.set_basis(lp.basis)
    except BaseException:
        solver.close()
        raise
    return solver, lp, plan["refactor_period"]


def check(solver, lp, label, started, pivots, device=False):
    """``device``: the preconditions from the rows the DEVICE makes of the basis (its own pivots, its inversion kernels) -- what the lists
    built by lu_device_tasks.hip hold -- and on the host's as well; else from ``lu_factor_host``, whose rows the handle was given."""
    basis = solver.basis()
    columns = lu_lps.basis_columns(lp.provider, basis)
    summary = lu_lps.preconditions(columns, lp.plant, planted=pivots == 0)
    exact, checks = exact_state(lp, basis)
    assert min(exact.x_exact) >= 0  # primal feasible, exactly
    report = {}
    assert_state(solver, exact, report=report, **checks)
    entered = len(set(int(c) for c in basis) - set(lp.basis.tolist()))
    print("%s: %s; %d entered columns in the basis; slots %r, inverse slots %r; %.1f s" % (
        label, ", ".join("%s %.1e" % item for item in sorted(report.items())), entered,
        [summary[name]["slots"] for name in lu_lps.LIST_NAMES], summary["inverse slots"], time.perf_counter() - started))
    if device:
        summary = lu_lps.preconditions(columns, lp.plant, planted=pivots == 0, factorise=device_factorisation, inverse_only=True)
        print("%s: the device's own rows: inverse slots %r, longest row %r, extra entries %r, classes %r" % (
            label, summary["inverse slots"], summary["inverse longest row"], summary["inverse extra entries"], summary["inverse classes"]))
    return exact


CASES = [(carry, m, 0, moment) for carry in (CARRY_LU, CARRY_LU_INVERSE) for m in (1024, 1025, 2048) for moment in "ac"] + \
        [(carry, 2049, period, moment) for carry in (CARRY_LU, CARRY_LU_INVERSE) for period in (0, 7, 63) for moment in "abcd"] + \
        [(CARRY_LU_INVERSE, m, 0, moment) for m in (4396, 4397, 5850) for moment in "ac"] + \
        [(CARRY_LU, m, 0, moment) for m in (4397, 8712) for moment in "ac"]


@pytest.mark.parametrize("carry, m, period, moment", CASES, ids=["%s-%d-period %d-%s" % (NAMES[c[0]], c[1], c[2], c[3]) for c in CASES])
def test_state_at_a_moment(carry, m, period, moment):
    started = time.perf_counter()
    if carry == CARRY_LU_INVERSE and m in (4396, 4397):  # the size at which the inverse-factor form gives up its fourth LDS vector
        assert lu_lps.last_size(True, period_of(carry, period, False) + 1, vectors=4) == 4396
    solver, lp, period = prepared(carry, m, period)
    try:
        pivots = pivots_of(moment, period)
        if pivots:
            assert solver.iterate(pivots) == (pivots, relp_amd.STOP_BUDGET)
        check(solver, lp, "%s %d period %d (%s)" % (NAMES[carry], m, period, moment), started, pivots)
    finally:
        solver.close()


@pytest.mark.parametrize("m, moment", [(m, moment) for m in (2049, 4397) for moment in "ad"])
def test_state_with_the_refactorisation_on_the_device(m, moment):
    """``lu_device_tasks.hip`` builds the compact records of the same lists from what ``lu_factor.hip`` left on the device.  The plant is
    "device" (tests/lu_lps.py): no row of the basis beyond the 256 entries the device's elimination takes -- with the full plant the host
    would factorise instead --, and a chain of 400 that gives U^-1 its rows beyond 256: the extra entries of the records."""
    started = time.perf_counter()
    solver, lp, period = prepared(CARRY_LU_INVERSE, m, device=True, plant="device")
    try:
        pivots = pivots_of(moment, period)
        if pivots:
            assert solver.iterate(pivots) == (pivots, relp_amd.STOP_BUDGET)
        check(solver, lp, "lu_inverse %d device refactorisation (%s)" % (m, moment), started, pivots, device=True)
        record = solver.record()  # (after ``check``: where the device gives up, ``lu_factor_device`` in there says with which status)
        assert record["lu_refactor"] == "device" and record["device_refactor_fallbacks"] == 0, record
    finally:
        solver.close()


def test_plain_launches_end_on_the_same_bits_across_a_refactorisation():
    """Moment (d) at 2049: the first batch is a full one and is replayed from a graph; with ``use_graph=0`` the same kernels are launched
    one by one.  Bit-equal x_B, the same basis -- and that state is the exact one."""
    started = time.perf_counter()
    results = []
    for use_graph in (1, 0):
        solver, lp, period = prepared(CARRY_LU, 2049, use_graph=use_graph)
        try:
            pivots = pivots_of("d", period)
            assert solver.iterate(pivots) == (pivots, relp_amd.STOP_BUDGET)
            results.append((solver.basis(), solver.b()))
            if not use_graph:
                check(solver, lp, "lu 2049 period %d (d), plain launches" % period, started, pivots)
        finally:
            solver.close()
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])


def test_a_position_that_leaves_twice_within_a_cycle():
    """The dead slot of the bordered form (lu.hpp: ``trail_pos = -1``, a zero row and column of T): moment (c) of the Forrest-Tomlin carry
    stepped with ``iterate(1)``, in which some basis position is pivoted on twice before the refactorisation; the batched walk ends on the
    same basis.  Seed 1000 + m gives 31 different positions (on the device and in the f64 model alike), so the seeds are tried from
    2000 + m on, as in ``sparse_lps``; 2000 + m gives two such positions."""
    started = time.perf_counter()
    m = 2049
    for seed in (2000 + m, 3000 + m, 4000 + m):
        solver, lp, period = prepared(CARRY_LU, m, seed=seed)
        try:
            rows = []
            for _ in range(period):
                assert solver.iterate(1) == (1, relp_amd.STOP_BUDGET)
                rows.append(solver.last_pivot()[2])
            stepped = solver.basis()
            if len(set(rows)) < len(rows):
                check(solver, lp, "lu 2049 seed %d period %d (c), stepped, %d positions twice" % (seed, period, len(rows) - len(set(rows))), started, period)
                break
        finally:
            solver.close()
    else:
        raise AssertionError("no seed gives a position that leaves twice")
    solver, lp, period = prepared(CARRY_LU, m, seed=seed)
    try:
        assert solver.iterate(period) == (period, relp_amd.STOP_BUDGET)
        assert np.array_equal(solver.basis(), stepped)
        check(solver, lp, "lu 2049 seed %d period %d (c), the same walk in one batch" % (seed, period), started, period)
    finally:
        solver.close()


# ---- the checks object to a wrong reference -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def at_2049():
    solver, lp, _ = prepared(CARRY_LU_INVERSE, 2049)
    yield solver, lp, exact_state(lp, solver.basis())[1]
    solver.close()


def test_the_state_of_a_basis_with_two_positions_of_an_arrow_exchanged_is_refused(at_2049):
    solver, lp, checks = at_2049
    arrow = np.flatnonzero(lp.region_of_row == lp.region_names.index("arrow 258"))  # (the widest: rows of 257 entries)
    first, second = [int(i) for i in arrow if i in set(lp.planted_rows)][:2]
    basis = solver.basis()
    basis[[first, second]] = basis[[second, first]]
    with pytest.raises(AssertionError, match="row of the inverse"):
        assert_state(solver, lp.provider.state(basis, 2), **checks)


def test_a_reference_with_a_wrong_last_row_is_refused_by_the_inverse_and_by_the_btran(at_2049):
    """Row m - 1 of the exact inverse replaced: the row itself differs, and so does every BTRAN (each has an entry there)."""
    solver, lp, checks = at_2049
    exact = lp.provider.state(solver.basis(), 2)
    m = exact.m
    inverse_row, right_multiply = exact.inverse_row, exact.right_multiply
    from basis_state import long_double
    wrong = np.zeros(m)
    wrong[m - 1], wrong[0] = 1.0 + inverse_row(m - 1)[0][m - 1], 0.5

    def wrong_row(k):
        return (wrong, np.zeros(m)) if k == m - 1 else inverse_row(k)

    def wrong_product(rows, values):
        weight = sum(float(v) for r, v in zip(rows, values) if r == m - 1)
        return right_multiply(rows, values) + weight * (long_double(wrong, 0 * wrong) - long_double(*inverse_row(m - 1)))
    exact.inverse_row = wrong_row
    with pytest.raises(AssertionError, match="row of the inverse"):
        assert_state(solver, exact, parts=("inverse",), **checks)
    exact.inverse_row = inverse_row
    exact.right_multiply = wrong_product
    with pytest.raises(AssertionError, match="btran"):
        assert_state(solver, exact, parts=("btran",), **checks)
    exact.right_multiply = right_multiply
    assert_state(solver, exact, parts=("inverse", "btran"), **checks)  # (and the true reference passes both)
