"""The CLI's chunk reader without a GPU: hpg-fastq_amd/host/hpgq_reader.c on
csrc/hpgq_fastq_text.c, driven by the stand-alone program
tests/sanitize/reader_main.c under ASan + UBSan (single-end, two mate files and
interleaved input at many chunk sizes and pread thread counts, --cg batch ends,
the pairing and format errors of DESIGN.md §2.7)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_reader_standalone_under_asan_ubsan(tmp_path):
    exe = tmp_path / "reader_main"
    r = subprocess.run(["make", "-C", os.path.join(HERE, "sanitize"), f"OUT={tmp_path}", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    # (the program writes its inputs into its working directory)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, cwd=tmp_path,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "reader_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
