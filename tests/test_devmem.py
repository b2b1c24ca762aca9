"""The device / pinned memory owners (flink_amd/csrc/gw_devmem.h) on the CPU, on their own.

tests/native/devmem.cpp includes the real header over tests/native/fake_hip/hip/hip_runtime.h,
a malloc-backed stand-in for the few HIP calls the header makes, with counters for live
blocks and synchronises and a "fail the k-th allocation from now" switch.  It is compiled
here with g++ under AddressSanitizer and UBSan (a stand-alone program; without the sanitizers
when their runtimes are missing, which the output says) and run once: all-or-nothing growth
of DevBuf and DevCols with every allocation of a growth failing in turn, reserve_discard's
empty state after a failure, moves, and no block left at exit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def compile_devmem(tmp):
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    linked = subprocess.run(["g++", *SANITIZE, probe, "-o", os.path.join(tmp, "probe")], capture_output=True)
    flags = SANITIZE if linked.returncode == 0 else []
    print("devmem: compiled with " + " ".join(flags) if flags else
          "devmem: the sanitizer runtimes are missing, compiled without -fsanitize")
    exe = os.path.join(tmp, "devmem")
    # the stand-in hip/hip_runtime.h comes before any ROCm include path
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags,
                    "-I", os.path.join(ROOT, "tests", "native", "fake_hip"), "-I", os.path.join(ROOT, "flink_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "devmem.cpp"), "-o", exe], check=True)
    return exe


def test_owners_grow_all_or_nothing_and_free_once(tmp_path):
    r = subprocess.run([compile_devmem(str(tmp_path))], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]  # a failed check or a sanitizer report ends the program
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    assert [ln for ln in lines if ln.endswith("keep ok (1 columns)") or ln.endswith("keep ok (3 columns)")
            or ln.endswith("keep ok (4 columns)")] == lines[:3]
