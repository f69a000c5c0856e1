"""Cost of pnr_get_link_states (PioneerVectorEnv.link_states): time per call at N envs (default 65 536 and 1 048 576) for the
kinematic handle's own joints (NULL source: r, v from the state planes) and for a caller's [N, 12] joint buffer, into a
preallocated output.  Device events around K back-to-back calls after a warm-up, the median of ROUNDS; each size also
replays the K calls from a captured graph (no host work between launches).  The achieved rate is counted against
(572 + 48) B per env — the records written plus the q, qd a caller's buffer holds; the NULL source reads 96 B of state
planes per env instead of 48, so its true traffic is 668 B.  Usage: python tools/link_state_cost.py [N ...] [--rounds R]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import PioneerVectorEnv  # noqa: E402

BYTES_PER_ENV = 572 + 48
HBM_PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int, default=[65536, 1048576])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
args = ap.parse_args()
dev = torch.device("cuda:0")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, K):
    torch.cuda.synchronize()
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / K * 1e3            # us per call


res = []
for n in args.sizes:
    env = PioneerVectorEnv(n, device=dev, seed=0)
    env.reset()
    out = torch.empty((n, 11, 13), dtype=torch.float32, device=dev)
    js = torch.randn((n, 12), dtype=torch.float32, device=dev)
    calls = {"null_source": lambda: env.link_states(out=out), "joint_state": lambda: env.link_states(js, out=out)}
    row = {"envs": n, "bytes_per_env": BYTES_PER_ENV}
    for name, fn in calls.items():
        for _ in range(20):
            fn()
        eager = sorted(timed(fn, args.calls) for _ in range(args.rounds))
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            fn()                                     # warm-up on the capture stream
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                for _ in range(args.calls):
                    fn()
        torch.cuda.synchronize()
        g.replay()
        graph = sorted(timed(g.replay, 1) / args.calls for _ in range(args.rounds))
        us_e, us_g = eager[len(eager) // 2], graph[len(graph) // 2]
        row[name] = {"us_per_call_eager": us_e, "us_per_call_graph": us_g, "all_eager_us": eager, "all_graph_us": graph,
                     "TBps_graph": n * BYTES_PER_ENV / (us_g * 1e-6) / 1e12,
                     "frac_of_8TBps_graph": n * BYTES_PER_ENV / (us_g * 1e-6) / HBM_PEAK}
        del g
    res.append(row)
    print(json.dumps(row), flush=True)
    env.close()
