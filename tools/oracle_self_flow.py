"""The CPU oracle against ITSELF: how many instances of a workload change control flow (iteration, outer-iteration, rollout counts,
status), and by how much their solutions move, when the inputs move by one part in 1e15 — the share of a batch whose path rounding
alone decides (the measure behind test_synth32_tight11_against_the_oracle's control-flow bar; profiles/r07_parity.txt). x1 is
perturbed (synth32's ū is 0), and ū too where it is not zero. No GPU.
usage: python tools/oracle_self_flow.py [config] [batch] [--generator {pcg64,splitmix64}] [--offset N]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ilqr_amd_loader import load_package
from oracle import oracle

ap = argparse.ArgumentParser()
ap.add_argument("config", nargs="?", default="synth32_tight11")
ap.add_argument("batch", nargs="?", type=int, default=512)
ap.add_argument("--generator", choices=("pcg64", "splitmix64"), default="splitmix64")
ap.add_argument("--offset", type=int, default=0)
args = ap.parse_args()
pkg = load_package()
W = pkg.workloads
model, T, x1, ub = W.make_inputs(args.config, args.batch, offset=args.offset, generator=args.generator)
opts = oracle.default_options(**W.CONFIG_OPTIONS.get(args.config, {}))
threads = int(os.environ.get("ORACLE_THREADS", "16"))
r = oracle.solve_batch(model, T, x1, ub, options=opts, nthreads=threads, want_policy=False)
p = oracle.solve_batch(model, T, x1 * (1 + 1e-15), ub * (1 + 1e-15), options=opts, nthreads=threads, want_policy=False)
B = args.batch
same = np.logical_and.reduce([r["stats"][f] == p["stats"][f] for f in ("iterations", "outer_iterations", "rollouts", "status")])
dx = np.abs(p["x"] - r["x"]).reshape(B, -1).max(1)
du = np.abs(p["u"] - r["u"]).reshape(B, -1).max(1)
d = p["stats"]["iterations"] - r["stats"]["iterations"]
print("%s %s B=%d offset=%d: the oracle against itself with x1, ū x (1 + 1e-15): control flow identical on %d of %d instances; "
      "max |dx| %.2e where it is, max |dx| %.2e |du| %.2e where it is not; iteration differences there %s"
      % (args.generator, args.config, B, args.offset, same.sum(), B, dx[same].max(initial=0.0), dx[~same].max(initial=0.0),
         du[~same].max(initial=0.0), sorted(d[~same].tolist())))
