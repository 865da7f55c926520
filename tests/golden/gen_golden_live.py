#!/usr/bin/env python3
"""Record the worlds of tests/test_oracle_live_reference.py from the UNMODIFIED reference (where its tree is present; import
recipe in gen_golden.py): the recorders of gen_golden.py / gen_golden_scenarios.py / gen_golden_shapes.py on seeds that none
of the other fixtures hold (derived from one day stamp, BASE), with the squeezes and action mixes those recorders use.

    python tests/golden/gen_golden_live.py            # rewrites tests/golden/live_*.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import gen_golden as gg  # noqa: E402  (sets up the stub gym + reference import path)
import gen_golden_scenarios as gs  # noqa: E402
import gen_golden_shapes as gsh  # noqa: E402

BASE = 261015      # the day stamp (yymmdd) the worlds were drawn for


def main():
    base = BASE * 100
    jobs = {
        "simple": gg.record("simple", gg.make_env("simple"), [base + k for k in range(6)], 30),
        "simple_spread": gg.record("simple_spread", gg.make_env("simple_spread", benchmark=True), [base + 10 + k for k in range(9)], 20,
                                   squeeze_every=3, arng=np.random.RandomState(base)),
        "simple_tag": gg.record("simple_tag", gg.make_env("simple_tag", benchmark=True), [base + 30 + k for k in range(9)], 20,
                                squeeze_every=3, squeeze=0.25, arng=np.random.RandomState(base + 1)),
        "simple_spread_n7": gg.record("simple_spread_n7", gg.spread_n(7), [base + 50 + k for k in range(4)], 8, squeeze_every=2,
                                      squeeze=0.4, arng=np.random.RandomState(base + 2)),
    }
    base = BASE * 1000 + 7
    for k, (name, sq) in enumerate([("simple_adversary", 0), ("simple_push", 0), ("simple_speaker_listener", 0), ("simple_reference", 0),
                                    ("simple_crypto", 0), ("simple_world_comm", 8)]):
        jobs["f3_" + name] = gs.record(name, [base + 100 * k + j for j in range(64)], 6, squeeze_every=sq, stage=True)
    for k, (name, A, nadv) in enumerate(gsh.SHAPES):      # other team sizes: the reference's callbacks on resized agent lists
        jobs["shape_%s_%d_%d" % (name, A, nadv)] = gs.record(
            name, [base + 1000 + 100 * k + j for j in range(32)], 4, squeeze_every=8 if name == "simple_world_comm" else 0,
            stage=True, env_factory=gsh.factory(name, A, nadv))
    for name, data in jobs.items():
        data = dict(data, live_seed=np.int64(BASE))
        np.savez_compressed(os.path.join(HERE, "live_" + name + ".npz"), **data)
        print("live_%s.npz" % name)


if __name__ == "__main__":
    main()
