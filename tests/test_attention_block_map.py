"""The attention block map (megatron_amd/ops/csrc/attention_sched.h) on the
host: attention_block_map_check.cpp includes the header as plain C++ and walks
every grid id over a table of (nblk, ngrp, rep, heavy_last).  A block that the
map never produces is a block that is never computed, which a GPU compare can
miss when the output tensor happens to reuse memory that holds the right
values; this exhaustive check cannot."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "megatron_amd", "ops", "csrc")


def test_block_map_exhaustive(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "attention_block_map_check")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
         os.path.join(HERE, "attention_block_map_check.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # 20 nblk x 40 ngrp x 3 rep x 2 orders
    assert r.stdout.strip() == "OK 4800", r.stdout
