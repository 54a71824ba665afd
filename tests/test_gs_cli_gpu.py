"""`hpg-fastq signature` on the GPU: the file it writes is the genomic signature
of tests/gs_ref.py whatever the chunk size, and `stats --cg --gs-filename`
reads it."""
import os
import struct

import numpy as np
import pytest

import gs_ref
import hpgfastq as H
from cli_lib import run_cli

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 7


@pytest.fixture(scope="module")
def signature_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gs_cli")
    text = gs_ref.fasta_np(17, 3 << 20, width=60, n_frac=0.005, lower=0.2, iupac=0.01,
                           rec_bases=700000, header=b">chr ACGTN test\n")
    fa = d / "ref.fa"
    fa.write_bytes(text)
    one, many = d / "one", d / "many"
    r1 = run_cli(["signature", "-f", fa, "-o", one, "--k", K])
    r2 = run_cli(["signature", "-f", fa, "-o", many, "--k", K, "--chunk-mb", 1])
    return text, one / f"ref.fa_k={K}.fg", many / f"ref.fa_k={K}.fg", r1, r2


def test_one_piece_or_several(signature_files):
    text, f1, f2, r1, r2 = signature_files
    table, info = gs_ref.fast(text, K)
    assert info["sequences"] >= 4 and info["ns"] > 0
    b1, b2 = f1.read_bytes(), f2.read_bytes()
    assert b1[180:] == b2[180:]                  # (the first 180 bytes hold the file's own name)
    dim = 1 << K
    assert len(b1) == 196 + 4 * dim * dim
    assert struct.unpack("<4I", b1[180:196]) == (K, dim, dim, info["words"])
    for f in (f1, f2):
        t, w = H.cgr_load_gs(str(f), K)
        np.testing.assert_array_equal(t.reshape(dim, dim), table)
        assert w == info["words"]
    for r in (r1, r2):
        for label, key in (("Num. sequences", "sequences"), ("Num. bases (ACGT)", "bases"),
                           ("Num. N", "ns"), ("Num. words", "words")):
            line = [x for x in r.stdout.splitlines() if x.startswith(label)]
            assert line and int(line[0].split(":")[1]) == info[key], label


def test_gs_filename_and_quiet(signature_files, tmp_path):
    text, f1, _, _, _ = signature_files
    out = tmp_path / "named.fg"
    r = run_cli(["signature", "-f", f1.parent.parent / "ref.fa", "--k", K, "--gs-filename", out, "--quiet"])
    assert r.stdout.strip() == ""
    assert out.read_bytes()[180:] == f1.read_bytes()[180:]


def _stats_with(gs_file, fq, k, out):
    words = struct.unpack("<I", gs_file.read_bytes()[192:196])[0]
    r = run_cli(["stats", "-f", fq, "-o", out, "--cg", "--k", k, "--gs-filename", gs_file])
    assert r.returncode == 0
    name = os.path.basename(str(fq))
    txt = (out / f"{name}.chaos_game.txt").read_text()
    assert f"Genomic signature file: {gs_file} ({words} words)" in txt
    assert "Diff matrix mean" in txt
    for suffix in ("_FG.pgm", "_QQ.pgm", "_FG_dif.pgm"):
        assert (out / f"{name}_k={k}{suffix}").exists(), suffix


def test_stats_reads_the_signature(signature_files, tmp_path):
    """signature -> stats --cg --gs-filename: the difference statistics name the
    file's word count and all three images are written.  At k = 7 the reads
    come from a FASTQ written here: tests/golden/kat_cgr.fq (reads of 4, 1 and 2
    bases) holds no 7-base word, and the difference table of a FASTQ without
    words is an error (hpgq_cgr_table_dif; LOG_FATAL in the reference).  The
    golden file makes the same trip at k = 2, where it has words."""
    text, f1, _, _, _ = signature_files
    rng = np.random.default_rng(2)
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for i in range(50):
            s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 100)].tobytes()
            f.write(b"@r%d\n" % i + s + b"\n+\n" + b"I" * 100 + b"\n")
    out7 = tmp_path / "k7"
    out7.mkdir()
    _stats_with(f1, fq, K, out7)
    out2 = tmp_path / "k2"
    run_cli(["signature", "-f", f1.parent.parent / "ref.fa", "-o", out2, "--k", 2, "--quiet"])
    gs2 = out2 / "ref.fa_k=2.fg"
    t, w = H.cgr_load_gs(str(gs2), 2)
    table, info = gs_ref.fast(text, 2)
    np.testing.assert_array_equal(t.reshape(4, 4), table)
    assert w == info["words"]
    _stats_with(gs2, os.path.join(GOLD, "kat_cgr.fq"), 2, out2)
