"""Mate pairs in the GPU parser: the de-interleaving parse against the
single-text parser on the same records split into two texts (byte for byte),
and the mate-name check against the rule restated in tests/pairs_lib.py, with
two parsers and in interleaved form."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    """One engine (for its stream and its device -> host copies) and three
    parsers on that stream: two single-text ones and one for interleaved text."""
    with H.Engine(H.stats_params(lmax=150)) as e:
        with H.Parser(stream=e.stream) as p1, H.Parser(stream=e.stream) as p2, H.Parser(stream=e.stream) as pi:
            yield e, p1, p2, pi
            for p in (p1, p2, pi):
                p.set_max_workgroups(0)


def _fixed(lengths, seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for L in lengths:
        s = rng.choice(np.frombuffer(b"ACGTN", np.uint8), L).tobytes()
        q = (33 + rng.integers(0, 42, L)).astype(np.uint8).tobytes()
        pairs.append((s, q))
    return O.Reads.from_pairs(pairs)


@pytest.fixture(scope="module")
def synth_pairs():
    return (O.synth(5000, seed=41, L=150, trunc_pct=50), O.synth(5000, seed=42, L=150, trunc_pct=50))


SHAPES = {
    "one_pair": ([37], [52]),
    # (not the last record of its own text: a text ending in an empty line is trimmed there)
    "zero_length_mate_1": ([0, 12], [5, 9]),
    "zero_length_mate_2": ([12, 3], [0, 9]),
    "alternating_1_1000": ([1] * 300, [1000] * 300),
    "around_the_wave": ([63, 64, 65, 129, 64, 63, 129, 65], [64, 65, 129, 63, 129, 64, 63, 65]),
}


def _check_split(gpu, r1, r2, crlf, cap=0):
    e, p1, p2, pi = gpu
    h1, h2 = PL.mate_headers(r1.n, 1), PL.mate_headers(r2.n, 2)
    rec1 = PL.records(r1, h1, crlf=crlf)
    rec2 = PL.records(r2, h2, crlf=crlf, plus_header=True)
    pi.set_max_workgroups(cap)
    b1, b2 = pi.parse_interleaved(PL.interleave(rec1, rec2))
    assert b1.num_reads == r1.n and b2.num_reads == r2.n
    got = [PL.fetch(e, b1), PL.fetch(e, b2)]
    longest = pi.max_length
    text_order = pi.records()
    # the reference: the already tested single-text parser on each mate's own text
    want = [PL.fetch(e, p1.parse(b"".join(rec1))), PL.fetch(e, p2.parse(b"".join(rec2)))]
    for m in range(2):
        assert got[m][2][0] == 0
        np.testing.assert_array_equal(got[m][2], want[m][2], err_msg=f"data_indices of mate {m + 1}")
        assert got[m][0] == want[m][0], f"seq of mate {m + 1}"
        assert got[m][1] == want[m][1], f"quality of mate {m + 1}"
    # ... which are the reads themselves
    assert got[0][0] == r1.seq.tobytes() and got[1][1] == r2.qual.tobytes()
    assert longest == max(p1.max_length, p2.max_length)
    # all 2 n records in text order
    starts = np.cumsum([0] + [len(x) for pair in zip(rec1, rec2) for x in pair])[:-1]
    np.testing.assert_array_equal(text_order["start"], starts.astype(np.uint32))
    assert pi.pair_check() == -1


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_deinterleave_matches_single_text_parser(gpu, shape, crlf):
    l1, l2 = SHAPES[shape]
    _check_split(gpu, _fixed(l1, 7), _fixed(l2, 8), crlf)


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("cap", [0, 1, 3])
def test_deinterleave_synthetic_pairs(gpu, synth_pairs, cap, crlf):
    """5,000 pairs of truncated reads: the two scans cross tile boundaries; with
    the workgroup cap at 1 and 3 every workgroup of the copy pass takes many
    records."""
    _check_split(gpu, synth_pairs[0], synth_pairs[1], crlf, cap=cap)


def test_interleaved_errors(gpu):
    _e, _p1, _p2, pi = gpu
    rec = PL.records(_fixed([5, 6, 7], 1), PL.mate_headers(3, 1))
    with pytest.raises(H.HpgqError) as err:
        pi.parse_interleaved(b"".join(rec))          # an odd record count
    assert err.value.code == H.E_PAIRING
    with pytest.raises(H.HpgqError) as err:
        pi.parse_interleaved(rec[0] + b"@r\nACGT\n+\nIII\n")   # quality shorter than the sequence
    assert err.value.code == H.E_FORMAT
    with pytest.raises(H.HpgqError) as err:
        pi.parse_interleaved(rec[0] + rec[1] + b"@x\nAC\n")    # not whole records
    assert err.value.code == H.E_FORMAT
    b1, b2 = pi.parse_interleaved(b"")
    assert b1.num_reads == 0 and b2.num_reads == 0 and pi.pair_check() == -1


# ---- the mate-name check ---------------------------------------------------------
def _run_names(gpu, h1, h2, crlf=False, cap=0):
    """first_bad of both forms for the header lines h1 / h2 (short fixed reads)."""
    _e, p1, p2, pi = gpu
    r1, r2 = _fixed([3 + i % 5 for i in range(len(h1))], 3), _fixed([2 + i % 7 for i in range(len(h2))], 4)
    rec1, rec2 = PL.records(r1, h1, crlf=crlf), PL.records(r2, h2, crlf=crlf)
    for p in (p1, pi):
        p.set_max_workgroups(cap)
    p1.parse(b"".join(rec1))
    p2.parse(b"".join(rec2))
    two = p1.pair_check(p2)
    inter = None
    if len(h1) == len(h2):
        pi.parse_interleaved(PL.interleave(rec1, rec2))
        inter = pi.pair_check()
    return two, inter


def _long(n, tail=b""):
    return (b"@" + (b"HWI-ST1234:88:C0XYZACXX:5:1101:" * 8)[:n - len(tail)] + tail)


NAME_CASES = {
    "slash_suffixes": (b"@read7/1", b"@read7/2", True),
    "no_suffix": (b"@read7", b"@read7", True),
    "wrong_way_round": (b"@read7/2", b"@read7/1", False),
    "slash1_on_both": (b"@read7/1", b"@read7/1", True),
    "slash2_on_both": (b"@read7/2", b"@read7/2", True),
    "slash1_slash3": (b"@read7/1", b"@read7/3", False),
    "digits_without_slash": (b"@read71", b"@read72", False),
    "suffix_only": (b"@/1", b"@/2", True),
    "suffix_after_different_names": (b"@a/1", b"@b/2", False),
    "comment_after_space": (b"@read7 first mate", b"@read7 second mate", True),
    "comment_after_tab": (b"@read7\tlane:1", b"@read7\tlane:2", True),
    "suffix_and_comments": (b"@read7/1 1:N:0", b"@read7/2\t2:N:0", True),
    "empty_names": (b"@", b"@", True),
    "empty_names_with_comments": (b"@ x", b"@\ty", True),
    "empty_against_name": (b"@", b"@a", False),
    "prefix_of_the_other": (b"@read7", b"@read70", False),
    "prefix_the_other_way": (b"@read70", b"@read7", False),
    "one_suffix_only": (b"@read7/1", b"@read7", False),
    "last_byte_differs": (b"@read7a", b"@read7b", False),
    "first_byte_differs": (b"@aead7", b"@bead7", False),
    "two_bytes_differ": (b"@read7/1", b"@reae7/2", False),
    "slash_differs": (b"@read7/1", b"@read7_2", False),
}
for _n in (15, 16, 17, 18, 31, 32, 33, 34, 200):
    NAME_CASES[f"len{_n}_equal"] = (_long(_n), _long(_n), True)
    NAME_CASES[f"len{_n}_suffix"] = (_long(_n, b"/1"), _long(_n, b"/2"), True)
    NAME_CASES[f"len{_n}_last_byte"] = (_long(_n, b"x"), _long(_n, b"y"), False)
    NAME_CASES[f"len{_n}_prefix"] = (_long(_n), _long(_n) + b"A", False)
    NAME_CASES[f"len{_n}_suffix_wrong"] = (_long(_n, b"/2"), _long(_n, b"/1"), False)


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("case", sorted(NAME_CASES))
def test_name_rule(gpu, case, crlf):
    a, b, ok = NAME_CASES[case]
    assert PL.in_step(a, b) is ok          # the restatement reads the case as its name says
    h1 = PL.mate_headers(2, 1) + [a] + PL.mate_headers(2, 1, first=3)
    h2 = PL.mate_headers(2, 2) + [b] + PL.mate_headers(2, 2, first=3)
    want = PL.first_bad(h1, h2)
    assert want == (-1 if ok else 2)
    assert _run_names(gpu, h1, h2, crlf=crlf) == (want, want)


@pytest.mark.parametrize("bad_at", [[0], [499], [120, 377], [0, 499], []])
def test_lowest_bad_pair_is_reported(gpu, bad_at):
    h1, h2 = PL.mate_headers(500, 1), PL.mate_headers(500, 2)
    for i in bad_at:
        h2[i] = b"@other%d/2 c" % i
    want = PL.first_bad(h1, h2)
    assert want == (bad_at[0] if bad_at else -1)
    assert _run_names(gpu, h1, h2) == (want, want)


@pytest.mark.parametrize("bad_at", [None, 2999, 1700])
def test_many_pairs_one_workgroup(gpu, bad_at):
    """3,000 pairs with the workgroup cap at 1: every lane takes a dozen pairs."""
    h1, h2 = PL.mate_headers(3000, 1), PL.mate_headers(3000, 2)
    if bad_at is not None:
        h1[bad_at] = h1[bad_at].replace(b"/1", b"/3")
    want = PL.first_bad(h1, h2)
    assert want == (-1 if bad_at is None else bad_at)
    assert _run_names(gpu, h1, h2, cap=1) == (want, want)


@pytest.mark.parametrize("n1,n2", [(7, 5), (5, 7), (0, 3)])
def test_unequal_record_counts(gpu, n1, n2):
    h1, h2 = PL.mate_headers(n1, 1), PL.mate_headers(n2, 2)
    assert PL.first_bad(h1, h2) == min(n1, n2)
    assert _run_names(gpu, h1, h2)[0] == min(n1, n2)
    # a name mismatch below the shorter count comes first
    if min(n1, n2) > 2:
        h2[1] = b"@zzz/2"
        assert _run_names(gpu, h1, h2)[0] == 1


def test_pair_check_needs_the_right_parses(gpu):
    _e, p1, p2, pi = gpu
    rec = PL.records(_fixed([4, 4], 1), PL.mate_headers(2, 1))
    p1.parse(b"".join(rec))
    with pytest.raises(H.HpgqError) as err:
        p1.pair_check()              # not an interleaved parse
    assert err.value.code == -7
    pi.parse_interleaved(b"".join(rec))
    with pytest.raises(H.HpgqError) as err:
        pi.pair_check(p2)            # an interleaved parse against a second parser
    assert err.value.code == -7
