"""What a handle owns outside the caller's arenas -- page-locked blocks, events, the two staging rings, the launches, the exchange's
allocations (csrc/host_res.h) -- over the life of every kind of handle: create and destroy, both rings wrapping, a refused
grl_replay_add_observed, staging that grows and is reused, every act form, one-rank data parallelism destroyed while connected, a
behaviour-cloning session open at destruction, refused creations.  Under AddressSanitizer + UBSan with leak detection at its
default, as a STAND-ALONE program with its own main (tests/csrc/handle_lifetime_check.cpp) that goes through include/grl.h only,
built exactly as tests/test_session_lifetime_sanitized.py builds its program (the emulation's page-locked blocks and events are
heap blocks, tests/hostemu/hostemu.h).  Host code only; nothing here touches a GPU or loads sanitized code into Python."""
import subprocess

from test_session_lifetime_sanitized import SANITIZE, compile_program


def test_handle_lifetimes_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "handle_lifetime_check")
    compile_program(exe, str(tmp_path), SANITIZE, program="handle_lifetime_check")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "163 checks, 0 failed" in out.stdout, out.stdout
