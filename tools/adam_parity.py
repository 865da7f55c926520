"""Record the parity figures of the whole on-device update: runs tests/test_gpu_adam.py's three-update test on the GPU
with MPE_ADAM_PARITY_OUT set, so that it writes, per parameter tensor, DeviceAdam's and float32 torch's largest deviation from the
float64 chain, the bound and the name the device reports, and adds what the figures are.

    python tools/adam_parity.py --out profiles/adam_parity.json
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
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_adam.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider",
                            "-k", "test_three_whole_updates_against_the_float64_chain"], env=dict(os.environ, MPE_ADAM_PARITY_OUT=got), cwd=ROOT)
        res = {}
        if os.path.exists(got):
            with open(got) as f:
                res = json.loads(f.read())
    res = dict({"workload": "simple_spread, 64 worlds, T = 5, three updates of 320 rows: Minibatches -> Trainable -> PpoLoss -> DeviceAdam, clip 0.5",
                "reference": "float64 chain: tests/_ppo_loss_ref.rule64, tests/_mlp_grad_ref.agent_grads64, tests/_adam_ref.step(float64)",
                "yardstick": "float32 torch modules, autograd, clip_grad_norm_ and torch.optim.Adam on the same GPU",
                "bound": "per parameter tensor max(4 x torch's deviation, 2 float32 ulps of the tensor's largest magnitude)"}, **res)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print("%d blocks, test exit code %d -> %s" % (len(res.get("blocks", [])), r.returncode, a.out))
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
