#!/usr/bin/env python3
"""CPU census of the order stages on C5-shaped walks (tests/order_stage_law.py: ER graph of 1 M vertices, mean degree 40, k = 8,
one walk per wave with the 448-candidate cap): per walk, the table finals and the share of them whose target is its bucket's
leader (stage_final's fast path), the stage recomputations and how many of them the in-place edit of the lowest invalidated
stage would take over.  usage: tools/order_census.py [walks] [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import order_stage_law as L  # noqa: E402

walks = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
res = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in L.census(walks=walks, seed=1).items()}
text = json.dumps(res, indent=1)
print(text)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(text + "\n")
