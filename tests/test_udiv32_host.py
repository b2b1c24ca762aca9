"""The 32-bit magic division and the lean pass-1 classification (flink_amd/csrc/gw_common.h:
make_udiv32 / udiv32, p1_lean) on the CPU, on their own.

tests/native/udiv32.cpp includes the real header over tests/native/fake_hip and is compiled
here with g++ under UBSan (a stand-alone program; without the sanitizer when its runtime is
missing, which the output says) and run once: udiv32 against `/` for every n < 2^32 with
divisors 2, 3 and 2000, at 0, 1, the neighbours of sampled multiples and 2^32 - 1 for divisors
1, 7, 500, 1000, 2^20, 86 400 000, 2^31 - 1, 2^31, 2^32 - 1 and divisors >= 2^32; and p1_lean
against a restatement with 128-bit `/` over random geometries and records at every boundary.
The full classify needs the device headers and is compared on the GPU (test_gpu_p1_paths.py)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=undefined", "-fno-sanitize-recover=all"]


def compile_udiv32(tmp):
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    linked = subprocess.run(["g++", *SANITIZE, probe, "-o", os.path.join(tmp, "probe")], capture_output=True)
    flags = SANITIZE if linked.returncode == 0 else []
    print("udiv32: compiled with " + " ".join(flags) if flags else
          "udiv32: the sanitizer runtime is missing, compiled without -fsanitize")
    exe = os.path.join(tmp, "udiv32")
    # the stand-in hip/hip_runtime.h comes before any ROCm include path; the HIP function
    # attributes of GW_HD mean nothing to g++
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", *flags,
                    "-D__host__=", "-D__device__=", "-D__forceinline__=inline",
                    "-I", os.path.join(ROOT, "tests", "native", "fake_hip"), "-I", os.path.join(ROOT, "flink_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "udiv32.cpp"), "-o", exe], check=True)
    return exe


def test_udiv32_and_lean_classification_match_plain_division(tmp_path):
    r = subprocess.run([compile_udiv32(str(tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])  # a failed check or a sanitizer report
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    assert sum(ln.endswith("every n < 2^32 ok") for ln in lines) == 3
    assert sum(ln.endswith("sampled ok") for ln in lines) == 14
    assert sum(ln.startswith("p1_lean ") and ln.endswith("records ok") for ln in lines) == 4
