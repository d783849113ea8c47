"""Record the launch traces of the training scenarios in tests/_launch_trace.py
into tests/golden/launch_traces.json (run on the GPU, at the commit whose
behaviour is to be pinned).

    python scripts/record_launch_trace.py              # write the golden file
    python scripts/record_launch_trace.py --check      # second run, reversed order: must
                                                       # reproduce the file (a trace that
                                                       # depends on run order or chance
                                                       # must not be pinned)
    python scripts/record_launch_trace.py --out FILE
"""
import argparse
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _launch_trace as LT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=LT.GOLDEN)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    names = list(LT.SCENARIOS)
    if a.check:
        names.reverse()
    traces, bad = {}, 0
    for name in names:
        traces[name] = tr = LT.run_scenario(name)
        count = collections.Counter(r[0] for r in tr)
        missing = [n for n in LT.REQUIRED[name] if n not in count]
        print(f"{name}: {len(tr)} launches", dict(sorted(count.items())), flush=True)
        if missing:
            print(f"  MISSING required launchers: {missing}", flush=True)
            bad += 1
    traces = {n: traces[n] for n in LT.SCENARIOS}
    # through JSON, so that what is compared is what the file holds
    traces = json.loads(json.dumps(traces))
    if a.check:
        with open(a.out) as f:
            gold = LT.decode(json.load(f))
        for name in LT.SCENARIOS:
            if traces[name] != gold[name]:
                bad += 1
                g, t = gold[name], traces[name]
                i = next((k for k, (x, y) in enumerate(zip(g, t)) if x != y), min(len(g), len(t)))
                print(f"DIFFERS {name}: {len(g)} vs {len(t)} launches, first at {i}:\n  "
                      f"{g[i] if i < len(g) else None}\n  {t[i] if i < len(t) else None}")
        print("check:", "FAILED" if bad else "reproduced")
    else:
        enc = LT.encode(traces)
        with open(a.out, "w") as f:
            json.dump(enc, f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {a.out}: {len(enc['calls'])} distinct calls, {os.path.getsize(a.out)} bytes")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
