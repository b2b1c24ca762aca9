"""The host side of the two-stream operators (flink_amd/csrc/gw_joinop.h) on the CPU, on its own.

tests/native/joinop.cpp includes the real header over tests/native/fake_hip/hip/hip_runtime.h,
the malloc-backed stand-in whose log shows which stream recorded and waited for which event.
It is compiled here with g++ under AddressSanitizer and UBSan (a stand-alone program; without
the sanitizers when their runtimes are missing, which the output says) and run once: the
pending-row buffer's all-or-nothing growth with every allocation failing in turn, draining in
parts, view and clear; the sticky error rule; the hand-off between a producer's stream and the
operator's, on an error path too, and a half-made stream object's destruction; the staged
ingest's chunks, single staging allocation and error return; and no block left at exit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def compile_joinop(tmp):
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    linked = subprocess.run(["g++", *SANITIZE, probe, "-o", os.path.join(tmp, "probe")], capture_output=True)
    flags = SANITIZE if linked.returncode == 0 else []
    print("joinop: compiled with " + " ".join(flags) if flags else
          "joinop: the sanitizer runtimes are missing, compiled without -fsanitize")
    exe = os.path.join(tmp, "joinop")
    # the stand-in hip/hip_runtime.h comes before any ROCm include path
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags,
                    "-I", os.path.join(ROOT, "tests", "native", "fake_hip"), "-I", os.path.join(ROOT, "flink_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "joinop.cpp"), "-o", exe], check=True)
    return exe


def test_row_buffer_error_rule_stream_handoff_and_staged_ingest(tmp_path):
    r = subprocess.run([compile_joinop(str(tmp_path))], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]  # a failed check or a sanitizer report ends the program
    assert r.stdout.splitlines() == ["RowBuf: growth ok (6 blocks)", "RowBuf: growth ok (5 blocks)", "RowBuf: drain ok",
                                     "OpError: ok", "OpStream: ok", "staged_ingest: ok", "ok"]
