"""examples/resume_chunks_c_abi.c, the way tests/test_examples.py runs the other example: plain C99 over include/readbouncer_amd.h
alone; three reads fed in four chunks each through rb_resume_batch, every row compared with rb_classify_batch on the concatenation."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "readbouncer_amd")
EXAMPLE = os.path.join(ROOT, "examples", "resume_chunks_c_abi.c")


def _build(tmp_path):
    exe = str(tmp_path / "resume_chunks_c_abi")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           EXAMPLE, "-L", LIBDIR, "-lreadbouncer_amd", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def test_resume_example_is_c99_and_links(tmp_path):
    """builds with or without a GPU; without one the program refuses loudly (exit code 2), it has no CPU path"""
    from readbouncer_amd import capi
    exe = _build(tmp_path)
    if capi.device_count() <= 0:
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert p.returncode == 2, (p.returncode, p.stdout, p.stderr)
        assert "no CPU fallback" in p.stderr


@pytest.mark.gpu
def test_resume_example_rows_equal_the_concatenation(tmp_path):
    exe = _build(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "12 rows, 0 differ" in p.stdout
    # the example shows something: the reference read is decided, the random one is not, the third changes its mind on the way
    rows = [l.split() for l in p.stdout.splitlines() if l.startswith("chunk ")]
    dec = {(int(r[1]), int(r[3].rstrip(":"))): int(r[-1]) for r in rows}
    assert [dec[(c, 0)] for c in range(4)] == [1, 1, 1, 1] and [dec[(c, 1)] for c in range(4)] == [0, 0, 0, 0]
    assert dec[(0, 2)] == 0 and dec[(3, 2)] == 1
