"""Record tests/golden/abi_messages.json: (return code, phf_last_error()) of every faulty call in tests/abi_message_cases.py, from the
library built in a checkout of the commit the messages are pinned to.

    python tests/golden/make_golden_abi_messages.py --tree /path/to/built/checkout

No GPU is needed: every call fails its argument checks, or has no rows, before a launch."""
import argparse
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--tree", required=True, help="checkout whose built pyhillfit_amd/lib/libpyhillfit_amd.so is recorded")
    ap.add_argument("--out", default=os.path.join(HERE, "abi_messages.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.dirname(HERE))
    m = importlib.import_module("pyhillfit_amd._lib")
    assert os.path.abspath(m.__file__).startswith(os.path.abspath(a.tree)), m.__file__
    import abi_message_cases
    res = abi_message_cases.run(m.load(), m)
    with open(a.out, "w") as f:
        json.dump({"abi_version": m.ABI_VERSION, "cases": res}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(res), a.out))


if __name__ == "__main__":
    main()
