"""The owning types of madsim_amd/csrc/device_mem.h (device buffer, page-locked buffer, event, stream) without a device: tests/cpp/device_mem_check.cpp
is compiled against the stand-in runtime of tests/cpp/fake_hip with AddressSanitizer and UBSan and run as a program of its own.  It asserts that
room() grows and never shrinks, that a failed room() leaves {nullptr, 0} and a later one succeeds, that a move leaves its source empty, that
reset() and the destructors release everything exactly once — and, for a struct shaped like a flight and its groups, that after a failure of the
k-th creation (every k) one more ensure() leaves every resource there: the case one pointer standing for a group of resources got wrong."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owning_types_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "device_mem_check")
    # (the sanitizers' runtimes linked statically: the program carries them, wherever in the library list it is loaded)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "fake_hip"), "-I" + os.path.join(ROOT, "madsim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "device_mem_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert lines[:4] == ["ok DevBuf", "ok PinnedBuf", "ok Event Stream", "ok group of 12 resources, a failure at each"], p.stdout
    assert lines[4].startswith("ok all released once: ") and "FAILED" not in p.stdout and "runtime error" not in p.stderr
