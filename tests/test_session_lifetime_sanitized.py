"""The lifetime of a behaviour-cloning and of a GAIL session -- query, begin, a call, losses, end; begin twice; a refused begin; a
handle destroyed with its session open; for GAIL also the reward pass and the statistics -- under AddressSanitizer + UBSan, as a
STAND-ALONE program with its own main (tests/csrc/session_lifetime_check.cpp) that goes through include/grl.h only and hands the
library heap blocks of exactly the queried sizes.  The library's translation units are compiled as conftest.hostemu_lib lists them
(g++, -DGRL_HOSTEMU, tests/hostemu) together with the program into ONE executable.  Host code only; nothing here touches a GPU
or loads sanitized code into Python.

Compile time, units side by side, measured once on the development machine: 23 s without the sanitizer flags, 87 s with them; the
compile's timeout is ten times the former."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "deep-rl-grasping_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
COMPILE_TIMEOUT = 10 * 23


def compile_program(exe, obj_dir, extra, program="session_lifetime_check"):
    """every csrc/*.hip and tests/csrc/<program>.cpp, compiled side by side and linked into `exe`"""
    units = [(os.path.join(CSRC, f), f[:-4]) for f in sorted(os.listdir(CSRC)) if f.endswith(".hip")]
    units.append((os.path.join(HERE, "csrc", program + ".cpp"), program))
    flags = ["-std=c++17", "-O1", "-g"] + extra + ["-DGRL_HOSTEMU", "-I", os.path.join(HERE, "hostemu"), "-I", os.path.join(ROOT, "include")]
    objs = [os.path.join(obj_dir, name + ".o") for _, name in units]
    procs = [subprocess.Popen(["g++"] + flags + ["-x", "c++", "-c", src, "-o", o]) for (src, _), o in zip(units, objs)]
    try:
        assert all(p.wait(timeout=COMPILE_TIMEOUT) == 0 for p in procs), "g++ failed"
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    subprocess.check_call(["g++"] + extra + objs + ["-o", exe], timeout=COMPILE_TIMEOUT)


def test_session_lifetimes_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "session_lifetime_check")
    compile_program(exe, str(tmp_path), SANITIZE)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "70 checks, 0 failed" in out.stdout, out.stdout
