"""The life of a TD3 handle -- create, train (policy and critic-only updates; the caller's rows and normals, device draws, one of
each), metrics, act at every row count, destroy; a handle destroyed without training; refused creations; the entry points a TD3
handle refuses -- at five shapes, under AddressSanitizer + UBSan with leak detection at its default, as a STAND-ALONE program with
its own main (tests/csrc/td3_lifetime_check.cpp) that goes through include/grl.h only and hands the library heap blocks of exactly
the queried sizes, built exactly as tests/test_session_lifetime_sanitized.py builds its program.  Host code only; nothing here
touches a GPU or loads sanitized code into Python."""
import subprocess

from test_session_lifetime_sanitized import SANITIZE, compile_program


def test_td3_lifetimes_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "td3_lifetime_check")
    compile_program(exe, str(tmp_path), SANITIZE, program="td3_lifetime_check")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert " checks, 0 failed" in out.stdout and int(out.stdout.split(" checks")[0].split()[-1]) >= 300, out.stdout
