"""Record the parity figures of the MLP input gradients: runs tests/test_gpu_mlp_dinput.py's parity test on the GPU
with MPE_MLP_DINPUT_PARITY_OUT set, so that every (case, window) appends, per agent, the kernel's and float32 torch autograd's
largest deviation from the float64 restatement and the bound, and folds the lines into one file with the window that comes closest
to its bound.

    python tools/mlp_dinput_parity.py --out profiles/mlp_dinput_parity.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what the host walk gave with k_mlp_grad's recompute as it stands: the reason the rule adds the bias last and cuts its sums in four
CHAINS = ("bias last, every sum four chains folded pairwise (host walk with the bias first and one chain per sum: tail_bias3_M65 window (0, 1) "
          "agent 1 9.95e-12 > 7.28e-12; bias last, one chain: critics_M1 window (55, 5) agent 1 3.16e-08 > 2.25e-08; as built: at most 0.47 of the bound)")


def fold(rows):
    worst = {"fraction": -1.0}
    for r in rows:
        for k, v in r["deviation"].items():
            f = v["kernel"] / v["bound"] if v["bound"] > 0 else 0.0
            if f > worst["fraction"]:
                worst = dict(v, fraction=f, case=r["case"], window=r["window"], agent=k)
    return {"device": "MI355X", "reference": "float64 restatement of THE MLP INPUT GRADIENT RULE (tests/_mlp_dinput_ref.rule64)",
            "yardstick": "float32 torch autograd with respect to the input, same modules, same GPU",
            "bound": "per agent's window max(4 x torch's deviation, 2 float32 ulps of the window's own largest magnitude)",
            "sums": CHAINS, "largest_fraction_of_bound": worst, "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        lines = os.path.join(d, "parity.jsonl")
        env = dict(os.environ, MPE_MLP_DINPUT_PARITY_OUT=lines)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_mlp_dinput.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider",
                            "-k", "test_parity_with_the_float64_restatement"], env=env, cwd=ROOT)
        rows = []
        if os.path.exists(lines):
            with open(lines) as f:
                rows = [json.loads(x) for x in f if x.strip()]
    with open(a.out, "w") as f:
        f.write(json.dumps(fold(rows)) + "\n")
    print("%d windows, parity test exit code %d -> %s" % (len(rows), r.returncode, a.out))
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
