"""The streaming history and its host mirror (host/lq_hist.c, host/lq_small.c)
against a plain array model, on the CPU: tests/mirror/mirror_test.c supplies
memcpy / malloc stand-ins for the runtime calls they make, is compiled here
with the address and undefined-behaviour sanitizers and run as a child
process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "liquid-dsp_amd", "host")


def test_history_mirror_against_model(tmp_path):
    exe = str(tmp_path / "mirror_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "liquid-dsp_amd", "csrc"),
                    "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(ROOT, "tests", "mirror", "mirror_test.c"),
                    os.path.join(HOST, "lq_hist.c"), os.path.join(HOST, "lq_small.c"), "-lm"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "mirror ok"
