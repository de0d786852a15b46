#!/usr/bin/env python3
"""Two builds of the library on the large case of scripts/coupler_time.py (C<n> atmosphere = land over a tripolar ocean, order 2, no
nest, no wave grid), alternating, one fresh process per measurement:

    python scripts/coupler_ab.py --parent OTHER_TREE [--branch THIS_TREE] [--rounds 11] [--runs 5] [--large 384 1440 1080]

A measurement is one process: load the package of that tree, make the handle, one warm-up run(), `runs` timed runs, the median of
their wall times and of the handle's own `run` phase.  Round i measures the parent, then the branch (the order swaps every round).
Reported: the median over the rounds for each build, the mean of the paired differences branch - parent and its standard error
(the standard deviation of the differences / sqrt(rounds)), and whether the branch is slower by more than twice that error.
Only entries both builds have are used."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root, size, runs):
    sys.path.insert(0, root)
    import __graft_entry__
    fg = __graft_entry__.load_package()
    fg._lib.require_gpu()
    sys.path.insert(0, os.path.join(HERE, "scripts"))
    import coupler_time as ct
    ni, nx, ny = size
    atm = ct.cubed_sphere(fg, ni)
    ocn, omask, ext = ct.ocean(fg, nx, ny, False)
    with fg.CouplerMosaic(atm, None, ocn, omask, ocn_south_ext=ext) as m:
        m.run()
        wall, phase = [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            m.run()
            wall.append((time.perf_counter() - t0) * 1e3)
            phase.append(m.phase_ms()["run"])
        st = m.stats()
    print(json.dumps(dict(wall=float(np.median(wall)), run=float(np.median(phase)), naxo=st["naxo"], naxl=st["naxl"], d2h=st["d2h_bytes"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--branch", default=HERE)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--large", type=int, nargs=3, default=[384, 1440, 1080])
    ap.add_argument("--child")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.large, args.runs)
    if not args.parent:
        ap.error("--parent is needed")
    res = {"parent": [], "branch": []}
    for i in range(args.rounds):
        order = ("parent", "branch") if i % 2 == 0 else ("branch", "parent")
        for who in order:
            root = os.path.abspath(args.parent if who == "parent" else args.branch)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--runs", str(args.runs), "--large"] + [str(v) for v in args.large],
                                 check=True, capture_output=True, text=True, timeout=300).stdout
            res[who].append(json.loads(out.strip().splitlines()[-1]))
            print(f"round {i + 1} {who}: {res[who][-1]}", file=sys.stderr, flush=True)
    lines = [f"## No nest, no wave grid: parent and branch, C{args.large[0]} atmosphere = land over a tripolar {args.large[1]} x {args.large[2]} ocean, order 2", "",
             f"{args.rounds} alternating rounds, one fresh process per measurement (handle, warm-up, {args.runs} runs, their median); ms.", "",
             "| | parent, median | branch, median | mean of branch - parent | standard error of the difference | slower by more than 2 SE |", "|---|---|---|---|---|---|"]
    verdict = True
    for key, name in (("wall", "run(), wall"), ("run", "run(), the handle's own phase time")):
        p, b = np.array([r[key] for r in res["parent"]]), np.array([r[key] for r in res["branch"]])
        d = b - p
        se = float(np.std(d, ddof=1) / np.sqrt(d.size))
        slower = bool(np.mean(d) > 2 * se)
        verdict = verdict and not slower
        lines.append(f"| {name} | {np.median(p):.3f} | {np.median(b):.3f} | {np.mean(d):+.3f} | {se:.3f} | {'YES' if slower else 'no'} |")
    same = all(r[k] == res["parent"][0][k] for r in res["parent"] + res["branch"] for k in ("naxo", "naxl", "d2h"))
    lines += ["", f"List lengths and the bytes run() copied to the host are the same in every measurement of both builds: {same} "
              f"({res['branch'][0]['naxo']} / {res['branch'][0]['naxl']} cells, {res['branch'][0]['d2h']} bytes)."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if not (verdict and same):
        sys.exit("the branch is slower than the parent, or the two disagree")


if __name__ == "__main__":
    main()
