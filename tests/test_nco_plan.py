"""The oscillator's phase plan (host/nco_plan.c) on its own, on the CPU:
tests/plan/nco_plan_test.c and the module are compiled here without HIP, with
the flags of tests/test_plan_module.py (address and undefined-behaviour
sanitizers, statically linked), and run as a child process.  That the two link
with nothing but libc and libm shows the plan needs no GPU; the program checks
plan lookups and the device table bit for bit against the stepped recurrence,
the period-cap fall-back, and orbits that wrap upward and downward."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "liquid-dsp_amd", "host")


def test_nco_plan_module_against_stepped_phase(tmp_path):
    exe = str(tmp_path / "nco_plan_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "liquid-dsp_amd", "csrc"),
                    "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(ROOT, "tests", "plan", "nco_plan_test.c"),
                    os.path.join(HOST, "nco_plan.c"), "-lm"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert out.stdout.strip().endswith("nco plan ok")
