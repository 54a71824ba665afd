"""The genomic-signature rule without a GPU: the two forms of tests/gs_ref.py
against each other, a hand-derived known answer, the relation to the CGR
accumulator (oracle/pyref.py cgr_fill) and the place where the two part, and
the no-device behaviour of the C-ABI and the `signature` command."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest

import gs_ref
import hpgfastq as H
from cli_lib import run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.parametrize("form", [gs_ref.loop, gs_ref.fast])
def test_known_answer(form):
    exp = json.load(open(os.path.join(GOLD, "gs_kat_expected.json")))
    text = open(os.path.join(GOLD, exp["text_file"]), "rb").read()
    assert text == b">s1 ACGT\nACgTN\nacG\n>s2\nTT\nT\n"
    for k, e in exp["k"].items():
        table, info = form(text, int(k))
        assert table.tolist() == e["table"], k
        assert info == {"words": e["words"], "bases": exp["bases"], "ns": exp["ns"],
                        "sequences": exp["sequences"]}, k
    assert exp["k"]["1"]["table"] == [[2, 2], [2, 4]] and exp["k"]["2"]["words"] == 7


def _odd_texts():
    return [b"", b">", b"\n", b">x", b">x\n", b"A", b"N", b"ACGT", b">a>b\nAC>GT\nAC\n",
            b"AC\r\nGT\r\n>h ACGTN\r\nNNAC", b"acgtnACGTNRYKM \t01\nacgt", b">h1\n>h2\n\n\nA\nC\nG\nT\n",
            b"ACG>TTT", b"\n\n>x\nAC\n>y"]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 7, 8])
def test_loop_equals_numpy_form(k):
    rng = random.Random(100 + k)
    texts = _odd_texts()
    for t in range(4):
        texts.append(gs_ref.fasta(rng, 3, 0, 2000, rng.choice([1, 7, 60, 61, 70]), crlf=(t == 1)))
    texts.append(gs_ref.fasta_np(k, 20000, width=60, n_frac=0.01, lower=0.3, iupac=0.05, rec_bases=3000))
    texts.append(b">h\n" + b"A" * 500 + b"\n" + b"N" * 300 + b"ACGT" * 5)
    for tx in texts:
        tl, il = gs_ref.loop(tx, k)
        tf, inf = gs_ref.fast(tx, k)
        np.testing.assert_array_equal(tl, tf)
        assert il == inf, tx[:40]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 7, 8])
def test_rule_equals_cgr_fill_per_record(k):
    """Without a run of 48-k toward-dim moves the integer cell is the (int)f
    cell: the rule equals cgr_fill called once per record (header dropped, case
    folded, class-4 bytes removed)."""
    rng = random.Random(7 * k)
    dim = 1 << k
    for t in range(3):
        tx = gs_ref.fasta(rng, 3, 0, 3000, rng.choice([60, 61, 70]), crlf=(t == 1))
        table, info = gs_ref.loop(tx, k)
        ts, tq, wc = [0] * (dim * dim), [0] * (dim * dim), 0
        for r in gs_ref.records(tx):
            ts, tq, wc = pyref.cgr_fill(k, 0, [(r, bytes(len(r)))], table_seq=ts, table_q=tq,
                                        word_count=wc)
        assert table.reshape(-1).tolist() == ts
        assert info["words"] == wc


def _run_text(seed, run):
    rng = random.Random(seed)
    return (bytes(rng.choice(b"ACGT") for _ in range(20)) + b"T" * run +
            bytes(rng.choice(b"ACGT") for _ in range(40)))


def test_rule_diverges_from_cgr_fill_after_a_long_run():
    """the signature is the integer cell, not the carried double
    recurrence.  20 random bases, a run of T, 40 random bases at k = 7: a run of
    48 (>= 48-k toward-dim moves, the double within rounding of dim but not yet
    dim) gives other cells than cgr_fill in every one of 20 draws.  A run of 60
    gives the same cells: from 54 moves on the state is exactly dim, every word
    is clamped to dim-1 and nudged by EPSILON, and the next base halves that
    away.  (The divergence lives in runs of about 41..53.)"""
    k = 7
    for seed in range(20):
        for run, differs in ((48, True), (60, False)):
            s = _run_text(seed, run)
            table, info = gs_ref.loop(b">x\n" + s + b"\n", k)
            ts, _, wc = pyref.cgr_fill(k, 0, [(s, bytes(len(s)))])
            assert info["words"] == wc == len(s) - k + 1
            assert (table.reshape(-1).tolist() != ts) == differs, (seed, run)


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device path")
def test_gs_open_without_device():
    h = C.c_void_p()
    assert H.lib.hpgq_gs_open(C.byref(h), 0, 7, None) == -5
    assert not h.value
    with pytest.raises(H.HpgqError) as e:
        H.Signature(7)
    assert e.value.code == -5


def test_gs_invalid_arguments():
    """HPGQ_E_INVALID before any device call."""
    h = C.c_void_p()
    for k in (0, 13, -1):
        assert H.lib.hpgq_gs_open(C.byref(h), 0, k, None) == -1
    assert H.lib.hpgq_gs_open(None, 0, 7, None) == -1
    assert H.lib.hpgq_gs_add_device(None, None, 0) == -1
    assert H.lib.hpgq_gs_add_host(None, b"", 0) == -1
    assert H.lib.hpgq_gs_sync(None) == -1
    assert H.lib.hpgq_gs_reset(None) == -1
    assert H.lib.hpgq_gs_read(None, None, None) == -1
    assert H.lib.hpgq_gs_debug_set_max_workgroups(None, 1) == -1
    H.lib.hpgq_gs_close(None)


def test_cli_print_params(tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b">a\nACGT\n")
    r = run_cli(["signature", "-f", fa, "-o", tmp_path, "--print-params"])
    assert r.stdout.split() == ["k=7", f"input={fa}", f"output={tmp_path}/ref.fa_k=7.fg"]
    r = run_cli(["signature", "-f", fa, "--k", 9, "--print-params"])
    assert "k=9" in r.stdout.split() and "output=./ref.fa_k=9.fg" in r.stdout.split()
    r = run_cli(["signature", "-f", fa, "--gs-filename", "x/y.fg", "--print-params"])
    assert "output=x/y.fg" in r.stdout.split()
    assert not list(tmp_path.glob("*.fg"))


def test_cli_missing_file_and_bad_k(tmp_path):
    r = run_cli(["signature", "-f", tmp_path / "absent.fa"], check=False)
    assert r.returncode != 0 and "not found" in r.stdout
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b">a\nACGT\n")
    for k in (13, 0):
        r = run_cli(["signature", "-f", fa, "--k", k], check=False)
        assert r.returncode != 0 and "--k must be in 1..12" in r.stdout
    r = run_cli(["signature"], check=False)
    assert r.returncode != 0
