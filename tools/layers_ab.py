#!/usr/bin/env python3
"""Per-layer A/B of bench.py --full --dump-layers files: tools/layers_ab.py ARM=file1,file2,... ARM=... [layer substring]
Prints, per launch, the median avg_us of each arm over its files and the spread (max - min) of the first arm."""
import json
import statistics
import sys


def main():
    arms, want = [], ""
    for a in sys.argv[1:]:
        if "=" in a:
            name, files = a.split("=", 1)
            arms.append((name, [json.load(open(f))["launches"] for f in files.split(",")]))
        else:
            want = a
    layers = [s["layer"] for s in arms[0][1][0]]
    print("| layer | " + " | ".join(f"{n} us" for n, _ in arms) + f" | spread of {arms[0][0]} | kernel of {arms[-1][0]} |")
    print("|---|" + "---|" * (len(arms) + 2))
    tot = [0.0] * len(arms)
    for i, layer in enumerate(layers):
        if want not in layer:
            continue
        cols = []
        for k, (_, runs) in enumerate(arms):
            v = [r[i]["avg_us"] for r in runs if i < len(r) and r[i]["layer"] == layer]
            m = statistics.median(v) if v else float("nan")
            tot[k] += m
            cols.append(f"{m:.2f}")
        first = [r[i]["avg_us"] for r in arms[0][1]]
        kern = arms[-1][1][0][i]["kernel"] if i < len(arms[-1][1][0]) else ""
        print(f"| {layer} | " + " | ".join(cols) + f" | {max(first) - min(first):.2f} | `{kern}` |")
    print("| sum | " + " | ".join(f"{t:.1f}" for t in tot) + " | | |")


if __name__ == "__main__":
    main()
