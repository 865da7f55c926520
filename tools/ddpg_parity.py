"""Record the parity figures of the off-policy update's device pieces: runs tests/test_gpu_ddpg.py on the GPU with
MPE_DDPG_PARITY_OUT set, so that it writes, per checked quantity, the largest fraction of its bound that the sweep reached (the
kernel's deviation from the float64 restatement over the bound), and adds what the figures are.

    python tools/ddpg_parity.py --out profiles/ddpg_parity.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        got = os.path.join(d, "parity.json")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_ddpg.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider",
                            "-k", "parity_bound or outside_inside or actor_loss"], env=dict(os.environ, MPE_DDPG_PARITY_OUT=got), cwd=ROOT)
        res = {}
        if os.path.exists(got):
            with open(got) as f:
                res = json.loads(f.read())
    res = dict({"workload": "the layouts L69, L22, L72, L32 of tests/_ddpg_ref.py at M in {1, 63, 64, 65, 255, 256, 257, 1025}, reg_coef 0 and 1e-3; "
                            "ActorLoss on simple_spread, M = 65, Tanh nets",
                "reference": "the float64 restatements of tests/_ddpg_ref.py on the same float32 inputs; float64 torch autograd of the example's formula for ActorLoss",
                "yardstick": "float32 torch autograd on the same GPU",
                "bound": "max(4 x torch's deviation, 2 float32 ulps of the magnitude: the output's largest, for dlogits the operands' of g_j - dot); "
                         "rows_logp: 1e-5 on log p",
                "test_exit_code": r.returncode}, **res)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print("%d quantities, test exit code %d -> %s" % (len(res.get("fraction_of_bound", {})), r.returncode, a.out))
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
