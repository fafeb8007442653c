"""The tile-table builder and the host forms of csrc/q_wide_kernels.h (tests/hostemu/q_wide_ref1.h) under AddressSanitizer +
UBSan, as a STAND-ALONE program with its own main (tests/csrc/q_wide_check.cpp): ragged variables of 1, 255, 4097, 131 073 and
524 288 + 3 floats, every buffer a heap block of exactly the promised size.  Host code only; nothing here touches a GPU or loads
sanitized code into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tile_table_and_reference_forms_stay_inside_their_buffers_on_ragged_variables(tmp_path):
    exe = str(tmp_path / "q_wide_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DGRL_HOSTEMU", "-I", os.path.join(HERE, "hostemu"),
                           os.path.join(HERE, "csrc", "q_wide_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.count(": 0 mismatches") == 3, out.stdout
    assert "3 of 5 variables clipped" in out.stdout and "0 of 5 variables clipped" in out.stdout, out.stdout
