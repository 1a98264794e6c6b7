"""The owners of the library's buffers, streams and events (csrc/ss_owned.h) under ASan + UBSan, on the
CPU: tests/host/owned_main.cpp instantiates the buffer with a counting malloc policy and the handle
with a counting fake, in a stand-alone program that keeps its own live-allocation count -- grows,
moves, containers of owner structs, and a failure injected at every allocation of a function shaped
like the engine's group_room.  It must end with status 0, no report and nothing live."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "owned_main.cpp")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer runs belong on the CPU host")
def test_owned_sanitized(tmp_path):
    # the program links its own sanitizer runtime: a runtime preloaded into this process (the suite
    # under scripts/sanitize_cpu.sh) is not handed on to the compiler or to the program
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    exe = str(tmp_path / "owned_asan_ubsan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    SRC, "-o", exe], check=True, env=env)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    for mark in ("Sanitizer", "runtime error", "FAILED"):
        assert mark not in r.stderr, r.stderr[-4000:]
    assert "all checks held" in r.stdout
