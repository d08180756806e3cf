"""CPU proof that the tables of allreduce_abi_cases.py (run by test_allreduce_abi_gpu.py) are not
vacuous: the sizes really sit on both sides of the selector's thresholds (asked of the built library,
mscclppAmdSelectAlgo), the views really are unaligned / disjoint / guarded, the oracle's own output
passes the plain reference with no lane excluded, a wrong operand is seen by both judges, a wrong
operand order is seen by the bit-exact one, and the refused ranges really overlap."""
import numpy as np
import pytest

import allreduce_abi_cases as A
import collective_edge_cases as C
import oracle_lib as O


@pytest.fixture(scope="module")
def lib(built):
    import mscclpp_amd as m

    return m.lib()


def _regions(lib, n, group):
    return {A.selected(lib, n, r.nbytes, r.code) for r in A.rows(n) if r.group == group}


@pytest.mark.parametrize("n", A.RANKS)
def test_every_selector_region_has_rows_on_both_sides_of_each_threshold(lib, n):
    """The regions are the selector's own answers at the smallest and the largest message and one
    element below, at and above the two edges -- not a restated constant.  At 2 ranks the
    built-in table has two regions only (one-hop LL8 up to 1 MiB), so the 16 KiB edge changes nothing
    there; at 3 and 8 ranks it has three."""
    edges = (A.SMALL_EDGE, A.LARGE_EDGE)
    answers = {A.selected(lib, n, s, O.F32) for e in edges for s in (e - 4, e, e + 4)} | \
        {A.selected(lib, n, s, O.F32) for s in (4, A.MAX_MESSAGE)}
    assert len(answers) == (2 if n == 2 else 3)
    for group in (1, 2, 3):
        assert _regions(lib, n, group) == answers, group
    live = [e for e in edges if A.selected(lib, n, e, O.F32) != A.selected(lib, n, e + 1, O.F32)]
    assert live == list(edges[1:] if n == 2 else edges)
    for code, op in A.G1_TYPES:
        es = O.itemsize(code)
        sizes = A.threshold_sizes(es)
        assert all(Row in A.rows(n) for Row in (A.Row(1, code, op, s, f, None) for s in sizes for f in ("base", "inplace")))
        for e in live:
            below, at, above = (A.selected(lib, n, s, code) for s in (e - es, e, e + es))
            assert below == at != above, (code, e)
            assert {e - es, e, e + es} <= set(sizes)
        assert es in sizes and max(sizes) <= A.MAX_MESSAGE
    for code in A.G2_TYPES:
        assert {A.selected(lib, n, s, code) for s in A.region_sizes(O.itemsize(code))} == answers
    assert max(r.nbytes for r in A.rows(n)) <= A.MAX_MESSAGE
    assert max(ref.nbytes * (n if ref.what == "reducescatter" else 1) for ref in A.REFUSALS) <= A.MAX_MESSAGE


def test_the_table_has_what_the_groups_promise():
    rows = A.rows(8)
    assert len(set(rows)) == len(rows)
    assert {(r.code, r.op) for r in rows if r.group == 2} == {(c, op) for c in A.NCCL_TYPE for op in (O.SUM, O.MIN)}
    assert set(A.NCCL_TYPE) == {O.F16, O.BF16, O.F32, O.I32, O.U32, O.U8, O.E4M3, O.E5M2}
    assert all(r.form == "inplace" for r in rows if r.group == 2)
    assert {(r.form, r.code) for r in rows if r.group == 3} == {(f, c) for f in "abc" for c, _ in A.G3_TYPES}
    assert {(r.algo, r.form, r.code) for r in rows if r.group == 4} == \
        {(a, f, c) for a in A.FORCED for f in "bc" for c, _ in A.G4_TYPES}
    assert all(r.algo is None for r in rows if r.group != 4)
    for n in A.RANKS:
        for k in (1, 2, 3, 24):  # dealing the rows over process groups loses none
            dealt = [r for p in A.parts(n, k) for r in p]
            assert sorted(dealt) == sorted(A.rows(n)) and all(A.parts(n, k))
    # float MIN rows over bits carry the planted NaN / +-0 / subnormal / inf groups
    row = next(r for r in rows if r.group == 2 and r.code == O.F16 and r.op == O.MIN)
    ins = A.row_inputs(8, row, 0)
    nan = [(a & 0x7C00 == 0x7C00) & (a & 0x3FF != 0) for a in ins]
    assert any(m[0] for m in nan) and A.row_families(row) == ("bits", "finite", "bits")
    # every buffer of a row differs: the seed carries the row, the call and the rank
    other = next(r for r in rows if r.group == 3 and r.code == O.F16)
    bufs = [A.row_inputs(3, r, call)[rank][:64].tobytes() for r in (row, other) for call in range(A.CALLS)
            for rank in range(3)]
    assert len(set(bufs)) == len(bufs)


def test_views_are_unaligned_disjoint_and_guarded():
    for row in A.rows(8):
        (sa, so), (ra, ro), sizes = A.layout(row)
        es, nb = O.itemsize(row.code), row.nbytes
        assert so + nb + A.GUARD_BYTES <= sizes[sa] and ro + nb + A.GUARD_BYTES <= sizes[ra]
        if row.form == "c":
            assert (sa, so) == (ra, ro) and so % es == 0 and so % 16 != 0 and so >= A.GUARD_BYTES
        elif row.form == "b":
            assert sa == ra and so >= A.GUARD_BYTES and ro - (so + nb) >= A.GUARD_BYTES and so % 16 == 0 == ro % 16
        elif row.form == "a":
            assert sa != ra and so == ro == 272
        elif row.form == "inplace":
            assert (sa, so) == (ra, ro) == (0, 0)
        else:
            assert sa != ra and so == ro == 0


def test_refused_ranges_overlap_and_are_no_in_place_form():
    for n in A.RANKS:
        for ref in A.REFUSALS:
            for rank in range(n):
                s, sl, r, rl, total = A.refusal_layout(ref, rank, n)
                assert s < r + rl and r < s + sl                      # they overlap
                assert s >= A.GUARD_BYTES and max(s + sl, r + rl) + A.GUARD_BYTES <= total
                if ref.what == "allreduce":
                    assert r != s and sl == rl == ref.nbytes           # not send == recv
                else:
                    assert r != s + rank * ref.nbytes                   # not recv == send + rank * bytes
                    assert (r - s) % ref.nbytes == 0 and s <= r and r + rl <= s + sl  # a whole other block
    assert {(ref.what, ref.nbytes) for ref in A.REFUSALS} >= {("allreduce", 4096), ("allreduce", 256 << 10)}
    assert any(ref.what == "reducescatter" for ref in A.REFUSALS)


@pytest.mark.parametrize("n", A.RANKS)
def test_the_judges_accept_the_oracle_and_see_a_wrong_operand(lib, n):
    """Per row: on every call with a plain reference the oracle's own output of every rank passes it, no
    lane excluded; and with one rank's input taken from another seed the oracle's output differs from
    the expected bytes (and the plain reference rejects it where the row has one)."""
    for row in A.rows(n):
        algo = row.algo or A.selected(lib, n, row.nbytes, row.code)
        probe = 1 if row.code in C.FLOATS else 0  # the call the wrong operand is tried on: a finite one for floats
        for call in range(A.CALLS):
            if not (A.has_plain(row, call) or call == probe):
                continue
            ins = A.row_inputs(n, row, call)
            exp = A.oracle_outputs(lib, algo, row.code, row.op, ins, row.nbytes)
            if exp is not None and A.has_plain(row, call):
                for r in range(n):
                    bad = C.plain_failures(row.code, row.op, ins, exp[r].copy())
                    assert bad.size == 0, (A.row_name(row), call, r, bad[:8])
            if call != probe:
                continue
            wrong = list(ins)
            victim = (A.row_id(n, row) + 1) % n
            if row.op == O.MIN and ins[0].size == 1:  # one lane: only the rank that holds the minimum shows
                victim = int(np.argmin([a.view(np.int32)[0] for a in ins]))
            make = C.finite if A.row_families(row)[call] == "finite" else C.bits
            wrong[victim] = make(row.code, ins[0].size, A.row_id(n, row) ^ 0x5A5A, call, victim)
            if exp is not None:
                off = A.oracle_outputs(lib, algo, row.code, row.op, wrong, row.nbytes)
                for r in range(n):
                    assert C.mismatches(row.code, off[r].copy(), exp[r].copy()).size, (A.row_name(row), r)
                    if A.has_plain(row, call):
                        assert C.plain_failures(row.code, row.op, ins, off[r].copy()).size, (A.row_name(row), r)
            else:  # rsag_pipeline: the plain reference is the only judge, so it must be the one that sees it
                assert A.has_plain(row, call)
                ref = A.oracle_outputs(lib, "fullmesh", row.code, row.op, wrong, row.nbytes)
                assert C.plain_failures(row.code, row.op, ins, ref[0].copy()).size, A.row_name(row)
                good = A.oracle_outputs(lib, "fullmesh", row.code, row.op, ins, row.nbytes)
                assert C.plain_failures(row.code, row.op, ins, good[0].copy()).size == 0, A.row_name(row)


@pytest.mark.parametrize("n", (3, 8))
def test_bit_exactness_tells_a_wrong_sum_order(lib, n):
    """Float SUM rows of group 1: the oracle's two sum orders differ in a lane of the bits or the
    finite call.  A one-element message is the exception by construction: its only lane lies in slice
    0, whose two orders (own first then ascending / ring from own) are the same sequence."""
    seen = 0
    for row in A.rows(n):  # out of place and in place: the form is part of the seed, so the inputs differ
        if row.group != 1 or row.op != O.SUM or row.code not in C.FLOATS:
            continue
        if row.nbytes == O.itemsize(row.code):
            continue
        seen += 1
        differs = False
        for call in (0, 1):
            ins = A.row_inputs(n, row, call)
            a, b = (A.oracle_outputs(lib, "fullmesh", row.code, row.op, ins, row.nbytes, order=k) for k in (0, 1))
            differs = differs or any(C.mismatches(row.code, a[r].copy(), b[r].copy()).size for r in range(n))
        assert differs, A.row_name(row)
    assert seen == 2 * 2 * 6  # two float types x two forms x the six sizes above one element
