"""The host forms of csrc/ln_kernels.h (tests/hostemu/ln_kernels_ref1.h) under AddressSanitizer + UBSan, as a STAND-ALONE
program with its own main (tests/csrc/ln_kernels_check.cpp): widths 48 / 65 / 100, 1 and 17 rows, every buffer a heap block of
exactly the promised size.  Host code only; nothing here touches a GPU or loads sanitized code into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_reference_forms_stay_inside_their_buffers_on_the_tail_shapes(tmp_path):
    exe = str(tmp_path / "ln_kernels_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DGRL_HOSTEMU", "-I", os.path.join(HERE, "hostemu"),
                           os.path.join(HERE, "csrc", "ln_kernels_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.count(": 0 mismatches") == 12, out.stdout
