"""The path tables of abi_path_cases are honest: every row's declared path is what the dispatch rule
(mscclppAmdPullReduceTakesLL, which touches no device) answers for its collective, rank count and size
-- in the default environment and with MSCCLPP_AMD_PULL_LL_MAX_BYTES=0 --, every family has both paths
for both collectives, in place and (PreMulSum) with a device scalar, and the rows above the cutover
have references that are none of the operands.  The declared paths are written in the tables; the GPU
tests assert them against the communicator's account, this test against the rule, so neither a change
of the rule nor of a table can move a row to the other kernel unnoticed.

Non-vacuity of the "pull" mode: without the variable the small rows of that mode would take LL, i.e.
their path assertions would fail (test_without_the_variable_the_small_pull_rows_are_not_pull)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_path_cases as T
import pull_reduce_ll_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = {"pull": "MAXAVG", "int": "INT", "premul": "PREMUL"}


def file_rows(mode):
    """(family, n, row) of every row the three multi-process files run in that mode."""
    return [(fam, n, row) for fam, (table, ranks) in T.FILES.items() for n in ranks[mode]
            for row in T.rows_of_mode(table, mode)]


def rule_in_a_process(value, queries):
    """pull_reduce_takes_ll in a process of its own with the variable set to `value`, or unset for None
    (the library reads it once)."""
    code = ("import mscclpp_amd as m; "
            f"print([int(m.pull_reduce_takes_ll(c, n, b)) for c, n, b in {queries!r}])")
    env = {k: v for k, v in os.environ.items() if k != T.VARIABLE}
    if value is not None:
        env[T.VARIABLE] = value
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True, check=True)
    return [bool(int(x)) for x in out.stdout.strip().splitlines()[-1].strip("[]").split(",")]


def rule_here(m, row, n):
    return T.LL if m.pull_reduce_takes_ll(row.coll, n, T.nbytes_of(row, n)) else T.PULL


# ---- the tables are the files' ---------------------------------------------------------------------
def test_tables_hold_what_the_files_run():
    assert {fam for fam, _ in T.FILES.items()} == set(TABLES)
    for fam, (table, ranks) in T.FILES.items():
        assert table is getattr(T, TABLES[fam]) and set(ranks) == set(T.MODES)
        assert all(row.family == fam for row in table)
        for row in table:
            assert (row.ll_at == T.NEVER) if row.coll == T.REDUCE else set(row.ll_at) <= set(T.EVERY), row
            assert (row.scalar in ("imm", "dev")) == (fam == "premul"), row
            assert T.ll_row(row) in C.ROWS, row
        cut = T.part(table, "cutover")
        assert len(cut) == 4 and [r.count for r in cut] == [("cutover", 0), ("cutover", 1)] * 2
        assert T.rows_of_mode(table, T.PULL) == [r for r in table if r.part != "cutover"]
        assert [r for r, _ in T.cutover_rows(table, T.LL)] == cut and T.cutover_rows(table, T.PULL) == []
    assert T.MAXAVG_RANKS == {T.LL: (2, 4, 8), T.PULL: (2, 3, 4, 8)}  # "pull" also at an odd rank count
    assert T.INT_RANKS == T.PREMUL_RANKS == {T.LL: (2, 8), T.PULL: (2, 8)}
    # 4 types x (2 ops x 3 counts x 3 collectives + 3 again + 6 in place) + 4 mixed + graph + after_refused
    # + 5 regrouped + 4 at the cutover
    assert len(T.MAXAVG) == 4 * (18 + 3 + 6) + 4 + 1 + 1 + 5 + 4
    assert len(T.INT) == 8 * 3 * 2 + 1 + 5 + 1 + 4
    assert len(T.PREMUL) == 2 * 3 * 3 + 2 + 1 + 1 + 1 + 4
    # the rows the issue of the cutover names: one pair each
    names = {(r.family, C.row_name(T.ll_row(r)), r.coll, r.inplace, r.scalar) for t in (T.INT, T.PREMUL) for r in T.part(t, "cutover")}
    assert names == {("int", "i64-sum", T.ALLREDUCE, True, None), ("int", "i8-min", T.REDUCE_SCATTER, False, None),
                     ("premul", "bf16-premulsum", T.ALLREDUCE, False, "dev"),
                     ("premul", "f32-premulsum", T.REDUCE_SCATTER, True, "imm")}
    # the largest buffers: the send buffer of a ReduceScatter above the cutover, just over 1 MiB at 2 and 8
    # ranks and just over 2 MiB at 4 (four blocks of 512 KiB and an element)
    for n in (2, 4, 8):
        most = max(T.nbytes_of(row, k) * (k if row.coll == T.REDUCE_SCATTER else 1) for _, k, row in file_rows(T.LL)
                   if row.part == "cutover" and k == n)
        assert most - 4 * n <= (2 << 20 if n == 4 else 1 << 20) < most  # n blocks and n elements of 4 bytes at most


def test_the_files_use_the_tables_rank_counts():
    import test_int_reduce_multiprocess_gpu as ti
    import test_mixed_collectives_gpu as tm
    import test_premul_sum_multiprocess_gpu as tp
    import test_pull_reduce_multiprocess_gpu as tx

    def params(fn):
        return [mark.args[1] for mark in fn.pytestmark if mark.name == "parametrize"]

    assert tx.RANKS is T.MAXAVG_RANKS
    assert params(tx.test_max_and_avg_through_the_nccl_abi) == [[(p, n) for p in T.MODES for n in T.MAXAVG_RANKS[p]]]
    for mod, fn, ranks in ((ti, ti.test_int_reductions_through_the_nccl_abi, T.INT_RANKS),
                           (tp, tp.test_premul_sum_through_the_nccl_abi, T.PREMUL_RANKS)):
        assert sorted(params(fn), key=str) == sorted([list(T.MODES), list(ranks[T.LL])], key=str) and ranks[T.LL] == ranks[T.PULL]
    assert params(tm.test_every_collective_back_to_back_across_processes) == [list(T.MIXED_RANKS)]
    assert params(tm.test_every_launcher_back_to_back_in_process) == [list(T.INPROCESS_RANKS)]
    assert tm.COUNT == T.MIXED_COUNT and set(r.key for r in T.MIXED) <= set(tm.ENTRIES)
    assert len(set(tm.ENTRIES)) == len(tm.ENTRIES) == 11 + len(T.MIXED)
    assert tm.LL_ENTRIES == ("ar_max_ll", "rs_avg_ll", "ar_i64_sum_ll", "ar_premul_ll")


# ---- declared path == the rule's answer ---------------------------------------------------------------
def test_declared_paths_are_the_rules_answer_in_the_default_environment(built):
    import mscclpp_amd as m

    assert T.VARIABLE not in os.environ, "run the suite without " + T.VARIABLE
    checked = 0
    for fam, n, row in file_rows(T.LL):
        assert T.declared(row, n, T.LL) == rule_here(m, row, n), (fam, n, row)
        checked += 1
    for n in T.MIXED_RANKS:
        for row in T.MIXED:
            assert T.declared(row, n, T.LL) == rule_here(m, row, n), (n, row)
            assert row.key.endswith("_ll") == (T.declared(row, n, T.LL) == T.LL) and \
                (row.key.endswith("_pull") or row.coll == T.REDUCE) == (T.declared(row, n, T.LL) == T.PULL), row
            checked += 1
    # in process the row chooses its launcher: the "ll" rows are sizes the rule sends to LL, a Reduce is "pull"
    for n in T.INPROCESS_RANKS:
        for gi in (0, 1):
            for row in T.inprocess_rows(gi):
                assert T.declared(row, n, T.LL) == rule_here(m, row, n), (n, gi, row)
                if row.part == "ll":
                    assert T.declared(row, n, T.LL) == T.LL, row
                elif row.coll == T.REDUCE:
                    assert T.declared(row, n, T.LL) == T.PULL, row
                checked += 1
    assert checked > 500


def test_declared_paths_are_the_rules_answer_with_the_variable_at_zero(built):
    rows = [(n, row) for _, n, row in file_rows(T.PULL)]
    # ... and the ReduceScatter / AllReduce rows the in-process half gives to the pull launcher
    rows += [(n, row) for n in T.INPROCESS_RANKS for gi in (0, 1) for row in T.inprocess_rows(gi) if row.part == "pull"]
    assert all(T.declared(row, n, T.PULL) == T.PULL for n, row in rows)
    answers = rule_in_a_process("0", [(row.coll, n, T.nbytes_of(row, n)) for n, row in rows])
    assert len(answers) == len(rows) > 600 and not any(answers)


def test_without_the_variable_the_small_pull_rows_are_not_pull(built):
    """Non-vacuity of the "pull" mode: were its variable removed, every AllReduce / ReduceScatter row
    that the default rule sends to LL would fail its path assertion -- the declared "pull" is then not
    the rule's answer.  That is every such row at 2 to 4 ranks and all but the 100003-element ones at 8."""
    import mscclpp_amd as m

    assert T.VARIABLE not in os.environ
    for fam, (table, ranks) in T.FILES.items():
        for n in ranks[T.PULL]:
            rows = [row for row in T.rows_of_mode(table, T.PULL) if row.coll != T.REDUCE]
            moved = [row for row in rows if rule_here(m, row, n) != T.declared(row, n, T.PULL)]
            assert moved == [row for row in rows if n in row.ll_at]
            stay = [row for row in rows if row not in moved]
            assert len(moved) >= 15 and (not stay or (fam == "pull" and n == 8 and all(r.count == 100003 for r in stay)))
            # ... among them what the mode is there to restore
            parts = {row.part for row in moved}
            assert parts >= {"pull": {"main", "again", "in_place", "mixed", "graph", "regrouped"},
                             "int": {"main", "one_element", "communicator", "flag", "counter"},
                             "premul": {"main", "once", "communicator", "device", "graph"}}[fam]


# ---- both paths, everywhere ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(TABLES))
def test_every_family_has_both_paths_for_both_collectives(fam):
    table, ranks = T.FILES[fam]
    for n in sorted(set(ranks[T.LL]) | set(ranks[T.PULL])):
        ran = [(T.declared(row, n, mode), row) for mode in T.MODES if n in ranks[mode] for row in T.rows_of_mode(table, mode)]
        paths = T.MODES if n in ranks[T.LL] else (T.PULL,)  # 3 ranks: "pull" only
        for path in paths:
            for coll in (T.ALLREDUCE, T.REDUCE_SCATTER):
                rows = [row for p, row in ran if p == path and row.coll == coll]
                assert rows, (fam, n, path, coll)
                assert any(row.inplace for row in rows), (fam, n, path, coll, "in place")
            if fam == "premul":
                assert any(row.scalar == "dev" for p, row in ran if p == path), (n, path, "device scalar")
        if n in ranks[T.LL]:  # the default environment alone reaches both kernels, for both collectives
            default = [(T.declared(row, n, T.LL), row.coll) for row in table]
            assert {(p, c) for p, c in default if c != T.REDUCE} == {(p, c) for p in T.MODES for c in (T.ALLREDUCE, T.REDUCE_SCATTER)}
        assert any(row.coll == T.REDUCE for _, row in ran)


def test_in_process_rows():
    for gi in (0, 1):
        rows = T.inprocess_rows(gi)
        ll = [r for r in rows if r.part == "ll"]
        assert {r.coll for r in ll} == {T.ALLREDUCE, T.REDUCE_SCATTER}
        assert sorted((r.family, r.scalar) for r in ll) == [("int", None), ("premul", "dev")] and ll[0].code == T.I.I64
        pull = [r for r in rows if r.part == "pull"]
        assert sorted(r.coll for r in pull if r.family == "premul") == sorted(T.P.COLLS)
        assert [r.code for r in pull if r.family == "int"] == [T.I.I8]
        assert all(r.count == T.INPROCESS_COUNT and not r.inplace for r in rows)
    both = T.inprocess_rows(0) + T.inprocess_rows(1)
    assert {r.scalar for r in both if r.part == "pull" and r.family == "premul"} == {"imm", "dev"}
    assert {r.coll for r in both if r.part == "ll" and r.family == "int"} == {T.ALLREDUCE, T.REDUCE_SCATTER}


# ---- the rows above the cutover ---------------------------------------------------------------------
def above_the_cutover():
    """(id, row, n, seed) of every row one element above the cutover: the three files' and the mixed test's."""
    out = []
    for fam, (table, ranks) in sorted(T.FILES.items()):
        for row, seed in T.cutover_rows(table, T.LL):
            if row.count == ("cutover", 1):
                out += [(f"{row.key}-{n}", row, n, seed) for n in ranks[T.LL]]
    import collective_edge_cases as E

    for row in T.MIXED:
        if row.count == ("cutover", 1):
            out += [(f"{row.key}-{n}", row, n, E.case_id("mixed", n, row.key, 0) % 100000) for n in T.MIXED_RANKS]
    return out


ABOVE = above_the_cutover()


def test_rows_above_the_cutover_are_the_smallest_that_reach_the_pull_kernel():
    assert len(ABOVE) == 2 * 3 + 2 * 2 + 2 * 2 + 4 * 2
    for _, row, n, _ in ABOVE:
        es, most = T.itemsize(row), C.BUILTIN_MAX[(row.coll, C.measured_ranks(n))]
        assert most % es == 0 and T.nbytes_of(row, n) == most + es and row.ll_at == T.NEVER
        partner = row._replace(count=("cutover", 0))
        assert T.nbytes_of(partner, n) == most


@pytest.mark.parametrize("case", ABOVE, ids=[c[0] for c in ABOVE])
def test_rows_above_the_cutover_have_references_that_are_no_operand(case):
    _, row, n, seed = case
    lrow, count = T.ll_row(row), T.count_of(row, n)
    total = count * (n if row.coll == T.REDUCE_SCATTER else 1)
    xs, ss = T.make_case(row, n, total, seed)
    assert (ss is None) == (row.family != "premul")
    assert all(len(x) == total and x.dtype == C.bits_dtype(lrow) for x in xs)
    ref = C.reference(lrow, xs, ss)
    assert C.mismatches(lrow, ref, ref).size == 0
    # the result is no single rank's operand: a sum differs from each nearly everywhere, a selection from
    # each in a good part of the elements
    least = total // 2 if row.op in (C.SUM, C.AVG, C.PREMUL_SUM) else total // 4
    for r, x in enumerate(xs):
        assert C.mismatches(lrow, x, ref).size > least, (row, n, r)
    if ss is not None:  # ... nor the unscaled sum, nor every rank under one scalar
        assert C.mismatches(lrow, C.reference(lrow, xs, [np.float32(1.0)] * n), ref).size > least
        assert C.mismatches(lrow, C.reference(lrow, xs, [ss[0]] * n), ref).size > least
    # float sums where pull_reduce_ll_cases.order_case applies (three ranks and more): the own-first
    # order gives other bits than rank order on some rank r >= 2 -- in this row's own data (its seed is
    # chosen so: of 2^17 bf16 results only a few sit on such a rounding boundary) and in the planted lanes
    if C.is_float_sum(lrow) and lrow in C.ORDER_ROWS and n >= 3:
        assert any(C.mismatches(lrow, C.own_first(lrow, xs, ss, r), ref).size for r in range(2, n)), (row, n)
        oxs, oss = C.order_case(lrow, n)
        assert C.mismatches(lrow, C.own_first(lrow, oxs, oss, n - 1), C.reference(lrow, oxs, oss)).size > 0
