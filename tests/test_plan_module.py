"""The resampler's timing plan (host/resamp_plan.c) on its own, on the CPU:
tests/plan/plan_test.c and the module are compiled here without HIP, with the
address and undefined-behaviour sanitizers, and run as a child process.  That
the two link with nothing but libc and libm shows the plan needs no GPU; the
program checks plan lookups and both device table formats bit for bit against
the timing state machine stepped from each plan's origin."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "liquid-dsp_amd", "host")


def test_plan_module_against_stepped_timing(tmp_path):
    exe = str(tmp_path / "plan_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "liquid-dsp_amd", "csrc"),
                    "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(ROOT, "tests", "plan", "plan_test.c"),
                    os.path.join(HOST, "resamp_plan.c"), "-lm"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("plan ok")
