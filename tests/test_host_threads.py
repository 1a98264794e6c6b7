"""The library's host threads under sanitizers, on the CPU: tests/host/host_threads_main.cpp drives the
FASTQ reader ring, read_parallel (csrc/fq_reader.h) and CopyPool (csrc/host_threads.h) -- the same
headers the HIP library compiles -- in a stand-alone program with a malloc'ed "device".  It is built
once with ThreadSanitizer and once with ASan + UBSan and must end with status 0 and no report."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "host_threads_main.cpp")
SANITIZERS = {
    "tsan": ["-fsanitize=thread"],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer runs belong on the CPU host")
@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_host_threads_sanitized(tmp_path, san):
    # the program links its own sanitizer runtime: a runtime preloaded into this process (the suite
    # under scripts/sanitize_cpu.sh) is not handed on to the compiler or to the program
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    exe = str(tmp_path / f"host_threads_{san}")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", *SANITIZERS[san], SRC, "-o", exe], check=True, env=env)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    for mark in ("Sanitizer", "runtime error", "FAILED"):
        assert mark not in r.stderr, r.stderr[-4000:]
    assert "all checks held" in r.stdout
