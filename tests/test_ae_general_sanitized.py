"""The host code that builds geometry, borders and tap tables for the auto-encoder's general route (csrc/ae_geom.h) and the host
forms of its kernels (csrc/ae_general.h, tests/hostemu/ae_general_ref1.h) under AddressSanitizer + UBSan, as a STAND-ALONE program
with its own main (tests/csrc/ae_general_check.cpp): every kernel size and channel count of the supported domain at B = 2, every
buffer a heap block of exactly the size the plan allocates.  Host code only; nothing here touches a GPU or loads sanitized code
into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_geometry_borders_and_tap_tables_stay_inside_their_buffers_over_the_domain(tmp_path):
    exe = str(tmp_path / "ae_general_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DGRL_HOSTEMU", "-I", os.path.join(HERE, "hostemu"),
                           os.path.join(HERE, "csrc", "ae_general_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "checks, 0 failed" in out.stdout, out.stdout
