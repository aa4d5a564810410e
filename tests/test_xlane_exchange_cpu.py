"""The exchange form of the forward transform's lane-high transpose (csrc/fft512.h, XLANE = 2) on the host: the signed first
pass, the DFT-8 on inputs shifted by 4, the lane relabelling and the whole 64-lane data flow against the v_cndmask form, all
exact (tests/native/xlane_exchange_test.cpp); and the switch between the two forms refuses what is neither."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exchange_form_equals_the_cndmask_form_on_the_host(tmp_path):
    exe = tmp_path / "xlane_exchange_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "ie-ache_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "xlane_exchange_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "XLANE_EXCHANGE_OK" in r.stdout


def test_forward_path_switch_refuses_unknown_forms(ia):
    for bad in (0, 3, -1):
        with pytest.raises(ia.IeacheError):
            ia.debug_forward_path(bad)
    ia.debug_forward_path(1)
    ia.debug_forward_path(2)  # the default again
