"""Record the parity figures of the PPO loss head: runs tests/test_gpu_ppo_loss.py's parity test on the GPU with
MPE_PPO_LOSS_PARITY_OUT set, so that every case appends the kernel's and float32 torch autograd's largest deviation from the float64
restatement and the bound, and folds the lines into one file with, per output, the case that comes closest to its bound.

    python tools/ppo_loss_parity.py --out profiles/ppo_loss_parity.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what the parity test gave with __expf on the ratio path (an MI355X), the reason the rule uses the accurate expf there
RATIO_EXP = ("accurate expf (with __expf: spread_A3_M257 surr 4.689e-06 > 3.815e-06 and dlogits 1.601e-08 > 1.523e-08)")


def fold(rows):
    worst = {}
    for r in rows:
        for k, v in r["deviation"].items():
            if k == "logp":
                continue
            f = v["kernel"] / v["bound"] if v["bound"] > 0 else 0.0
            if f > worst.get(k, {"fraction": -1.0})["fraction"]:
                worst[k] = {"fraction": f, "case": r["case"], "kernel": v["kernel"], "torch_float32": v["torch_float32"], "bound": v["bound"]}
    return {"device": "MI355X", "reference": "float64 restatement of THE PPO LOSS RULE (tests/_ppo_loss_ref.rule64)",
            "yardstick": "the same loss in float32 torch autograd on the same GPU",
            "bound": "logp 1e-5; every other output max(4 x torch's deviation, 2 float32 ulps of the output's own largest magnitude)",
            "ratio_exp": RATIO_EXP, "largest_logp_deviation": max(r["deviation"]["logp"]["kernel"] for r in rows),
            "largest_fraction_of_bound": worst, "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        lines = os.path.join(d, "parity.jsonl")
        env = dict(os.environ, MPE_PPO_LOSS_PARITY_OUT=lines)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_ppo_loss.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider",
                            "-k", "test_parity_with_the_float64_restatement"], env=env, cwd=ROOT)
        with open(lines) as f:
            rows = [json.loads(x) for x in f if x.strip()]
    with open(a.out, "w") as f:
        f.write(json.dumps(fold(rows)) + "\n")
    print("%d cases, parity test exit code %d -> %s" % (len(rows), r.returncode, a.out))
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
