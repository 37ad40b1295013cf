"""Scene preparation on the CPU alone (csrc/host/scene_prep.hpp through tools/prep_check.cpp).

`make prep_check` links the check program from the host objects only - no HIP library on the link line, so that it links at all says that preparation
is HIP-free. The program runs every builder (flattening in both precisions, sampler tables, pair / quad nodes, any-hit start lists, shadow candidate
lists, tile trees over synthetic census rays) on the golden scenes and on two hand-built trees (a single-leaf root, a 96-deep one-sided chain) and
follows every child word, leaf word and list offset the kernels would follow: exit status 0 = all of them stay inside their arrays.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs_ray_toy_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_prep_check_on_the_golden_scenes():
    subprocess.check_call(["make", "-s", "-C", CSRC, "prep_check"])
    scenes = [os.path.join(GOLDEN, p, "scene.json") for p in ("", "fuzz416_43", "fuzz508_96")]
    run = subprocess.run([os.path.join(ROOT, "build", "prep_check", "prep_check")] + scenes, capture_output=True, text=True, timeout=120)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stderr
    assert "prep_check: ok" in run.stdout
