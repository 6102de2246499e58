#!/usr/bin/env python3
"""Are the kernels of two `hipcc -S --cuda-device-only` listings of rt_amd/csrc/kernels.hip the same, kernel by kernel?

    python tools/kernel_listing_diff.py before.s after.s

What a refactor of the host side (the dispatch, launch_plan.cpp) must leave alone.  Kernels are matched by symbol, their order
ignored: it follows the order in which the host code names the instantiations.  A kernel's text runs from its label to the end
of its .amdhsa_kernel descriptor; the one thing normalised is the function's ordinal in the listing inside local labels and the
comments that name them (.LBB<ordinal>_<block>, "Header=BB<ordinal>_<block>"), which moves with the order.  Prints the number
of kernels compared and differing; exits non-zero unless the symbol sets are equal and no kernel differs."""
import re
import sys


def kernels(path):
    text = open(path).read()
    found = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel\n", text, re.M | re.S):
        symbol = m.group(1)
        start = text.index(f"\n{symbol}:", 0, m.start()) + 1
        body = re.sub(r"BB\d+_", "BB_", text[start : m.end()])
        found[symbol] = re.sub(r"^(\.LBB_\d+:) +;", r"\1 ;", body, flags=re.M)  # (the comment's column depends on the label's length)
    return found


before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
only = sorted(set(before) ^ set(after))
for symbol in only:
    print(("only in " + (sys.argv[1] if symbol in before else sys.argv[2])) + ": " + symbol)
differing = [symbol for symbol in sorted(set(before) & set(after)) if before[symbol] != after[symbol]]
for symbol in differing:
    print("differs: " + symbol)
print(f"{len(set(before) & set(after))} kernels compared, {len(differing)} differing, {len(only)} without a partner")
sys.exit(1 if only or differing else 0)
