"""csrc/tx_grid.hpp on the CPU (host compilation by hipcc, no GPU): the workgroup count the fused transmit kernel is launched
with, over slots 1/2/4/8, pattern lengths 2..9 and 70000, and every launch size around the resident count and around the
large-launch threshold.  tests/host/tx_grid_host_test.cpp states the properties."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "tx_grid_host_test.cpp")


def _build(tmp_path_factory, name, *flags):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp(name) / "tx_grid_host_test")
    subprocess.run(["hipcc", "-O2", "-std=c++17", *flags, "-o", out, SRC], check=True)
    return out


def test_grid_choice_holds_its_properties_at_every_edge(tmp_path_factory):
    r = subprocess.run([_build(tmp_path_factory, "txgrid")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.strip().endswith("2016 cases, 0 violations")          # 4 slots x 9 patterns x 7 resident counts x 8 sizes


def test_the_properties_catch_the_former_formula(tmp_path_factory):
    """The launcher used to ask coprimality of g * slots: with slots = 8 and a pattern of length 4 that loop ends at one
    workgroup.  The same program built around that expression must report it -- a grid further than S + D below the unadjusted
    one -- and nothing at slots = 1, where the two agree.  (A launch that fits the resident count was never adjusted, so the
    "one trip" property holds for the former expression too.)"""
    r = subprocess.run([_build(tmp_path_factory, "txgrid_old", "-DTX_GRID_TEST_PARENT_FORMULA")], capture_output=True, text=True)
    assert r.returncode == 1
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")]
    assert any(ln.startswith("FAIL within SD of base: slots=8 SD=4 ") and ln.endswith(" g=1") for ln in fails)
    assert all(ln.startswith("FAIL within SD of base: ") for ln in fails)
    assert not any(" slots=1 " in ln for ln in fails)
