"""The host side of a filter's two list tables, checked without a GPU: readbouncer_amd/csrc/rb_list_tables.h -- the state a filter keeps
of a table, the whole decision of what a call does with it (the branch for a capturing stream among it, which no GPU test takes), the
remembered refusals and the repay inequality -- through a stand-alone C++ program, plain and under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readbouncer_amd", "csrc")


def build_program(tmp_path, sanitize):
    exe = str(tmp_path / ("test_list_tables" + ("_san" if sanitize else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_list_tables.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", (False, True))
def test_decision_repay_and_state(tmp_path, sanitize):
    run = subprocess.run([build_program(tmp_path, sanitize)], capture_output=True, text=True)
    assert run.returncode == 0 and "failures: 0" in run.stdout, run.stdout + run.stderr


def test_the_header_is_free_of_hip_and_the_engine_keeps_one_of_each():
    """the header compiles alone (no HIP), and the engine has one builder, one table_for and one memory query for both list tables"""
    header = open(os.path.join(CSRC, "rb_list_tables.h")).read()
    assert "hip_runtime" not in header and "rb_device.h" not in header
    engine = open(os.path.join(CSRC, "rb_engine.hip")).read()
    assert '#include "rb_list_tables.h"' in engine
    for once in ("static int dibf_list_table_build(", "static int list_table_for(", "static int dibf_list_table_download(", "rbtables::table_call("):
        assert engine.count(once) == 1, once
    for gone in ("dibf_wide_build", "wide_table_for", "wide_refusal_stands_locked", "f->wide_refused"):
        assert gone not in engine, gone
    assert "rb_list_tables.h" in open(os.path.join(CSRC, "Makefile")).read()
