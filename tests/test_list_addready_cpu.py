"""The resident form of a list-table slot (readbouncer_amd/csrc/rb_lists.h: encode_resident, decode_resident) without a GPU: the
stand-alone program tests/cpp/test_lists_resident.cpp, plain and under the address and undefined-behaviour sanitizers -- round trips
through the canonical form, where the offsets and the spares point, when a slot carries a flag, and a host emulation of the kernel's two
add paths."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", (False, True))
def test_resident_slot_layout(tmp_path, sanitize):
    exe = str(tmp_path / "test_lists_resident")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_lists_resident.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "failures: 0" in run.stdout, run.stdout + run.stderr
