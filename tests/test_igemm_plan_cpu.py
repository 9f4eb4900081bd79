"""The implicit-GEMM launch plan (mm-vqa_amd/csrc/igemm_plan.h) without a GPU.

tests/igemm_plan_main.cpp is compiled with the host compiler under the address and undefined-behaviour sanitizers and
run as a child process over the cases of tests/golden/igemm_plans.json.  Every descriptor pointer of a case is a dummy
address that points at nothing, so a plan that dereferenced one would stop the program.  The expectations were recorded
from the launcher as it was before the plan became a function of its own (the file's `recorded_from` says how, its
`format` how they are stored): instance, grid, LDS bytes, every GemmAux field, the split, the coefficient / finishing
launches, the tuner's candidates, and the code and text of every refusal must be exactly those.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mm-vqa_amd", "csrc")


def flat(d, pre=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(flat(v, pre + k + "."))
        else:
            out[pre + k] = v
    return out


def per_tile(v, i):
    return v["per_tile"][i] if isinstance(v, dict) else v


def expected_cases(golden):
    """[(case line, expected flat record)] of every family and tile"""
    cases = []
    for fam in golden["families"]:
        for i, tile in enumerate(fam["tiles"]):
            want = {k: per_tile(v, i) for k, v in fam["expect"].items()}
            if want.get("rc", 0) == 0 and "candidates" not in want:
                want = {**{k: per_tile(v, tile) for k, v in golden["defaults"].items()}, **want}
            name = f"{fam['name']}/t{tile}"
            cases.append((f"name={name} tile={tile} {fam['case']}", dict(want, name=name)))
    return cases


def test_every_plan_matches_the_recorded_one(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) on PATH")
    with open(os.path.join(ROOT, "tests", "golden", "igemm_plans.json")) as f:
        cases = expected_cases(json.load(f))
    assert len(cases) >= 400
    exe = str(tmp_path / "igemm_plan_main")
    # the sanitizer runtimes are linked into the program (clang's default; gcc needs the flags): a dynamic runtime
    # insists on being the first library loaded and would refuse to start wherever the environment preloads another
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    "-I", CSRC, os.path.join(ROOT, "tests", "igemm_plan_main.cpp"), "-o", exe], check=True, timeout=300)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MMVQA_")}
    out = subprocess.run([exe], input="".join(line + "\n" for line, _ in cases), env=env, text=True, capture_output=True,
                         timeout=120)
    assert out.returncode == 0 and not out.stderr, f"igemm_plan_main exit {out.returncode}:\n{out.stderr[-4000:]}"
    results = [flat(json.loads(line)) for line in out.stdout.splitlines()]
    assert len(results) == len(cases)
    wrong = []
    for (_, want), got in zip(cases, results):
        if got != want:
            keys = sorted(k for k in set(want) | set(got) if want.get(k) != got.get(k))
            wrong.append(f"{want['name']}: " + "; ".join(f"{k}: want {want.get(k)!r}, got {got.get(k)!r}" for k in keys))
    assert not wrong, f"{len(wrong)} of {len(cases)} plans differ:\n" + "\n".join(wrong[:20])


def test_plan_header_has_no_hip_dependency():
    for name in ("igemm_plan.h", "host_defs.h"):
        with open(os.path.join(CSRC, name)) as f:
            src = f.read()
        assert "hip_runtime" not in src and "#include \"common.h\"" not in src and "getenv" not in src, name
