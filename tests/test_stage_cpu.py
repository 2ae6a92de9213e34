"""The staging layout and the staged-output table of the query passes (readbouncer_amd/csrc/rb_stage.h) on a CPU:
tests/cpp/test_stage.cpp has its own main, checks a few thousand seeded layouts (alignment, no overlap, bounded padding) and the
copy-back of sub-batches on a block of host memory, and exits with the number of failed checks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_layout_and_staged_outputs(tmp_path):
    exe = str(tmp_path / "test_stage")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_stage.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "failures: 0" in run.stdout, run.stdout + run.stderr
