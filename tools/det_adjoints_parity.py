"""Writes profiles/det_adjoints_parity.json from the "[det]" lines of tests/test_gpu_train_deterministic.py (development aid).

    python tools/det_adjoints_parity.py [--log FILE] [--out FILE]

Without --log the GPU tests are run here (pytest -s) and their output parsed; with it, a kept output of such a run.  Per
single-adjoint case: the relative L2 of the gather (deterministic) and of the atomic form against the float64 restatement, of the
two forms against each other, and the share of output elements without a contribution; per tensor of the whole conditioner
backward: the two modes against each other."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = re.compile(r"\[det\] (.*): err_det=(\S+) err_atomic=(\S+) parity=(\S+) zero share=(\S+)")
WHOLE = re.compile(r"\[det\] conditioner backward \((.*)\) (.*): deterministic vs atomic relL2=([0-9.e+-]+)(?: \(atomic vs atomic ([0-9.e+-]+))?")


def parse(text):
    rows = []
    for m in CASE.finditer(text):
        rows.append({"case": m.group(1), "err_det": float(m.group(2)), "err_atomic": float(m.group(3)), "parity": float(m.group(4)),
                     "zero_share": float(m.group(5))})
    for m in WHOLE.finditer(text):
        rows.append({"case": f"conditioner backward, {m.group(1)}, {m.group(2)}", "parity": float(m.group(3))})
        if m.group(4):
            rows[-1]["atomic_run_to_run"] = float(m.group(4))
    return rows


def main():
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "det_adjoints_parity.json")
    if "--log" in args:
        text = open(args[args.index("--log") + 1]).read()
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_train_deterministic.py", "-q", "-s", "-m", "gpu"], cwd=ROOT,
                           capture_output=True, text=True)
        text = r.stdout
        print(text[-400:])
    rows = parse(text)
    if not rows:
        raise SystemExit("no [det] lines found")
    what = ("gather (deterministic) vs atomic form of the conditioner's three gather adjoints on one MI355X: relative L2 of each form "
            "against the float64 restatement (err_*), of the two forms against each other (parity), and the share of output elements "
            "without a contribution; tests/test_gpu_train_deterministic.py, written by tools/det_adjoints_parity.py")
    with open(out, "w") as f:
        json.dump({"what": what, "rows": rows}, f, indent=1)
    print(f"{len(rows)} rows -> {out}")


if __name__ == "__main__":
    main()
