#!/usr/bin/env python3
"""sha256 of every translation unit's device code, to compare two trees.

    python tools/device_hash.py OUT.json      # this tree
    python tools/device_hash.py A.json B.json # compare two results

Each unit of dragonboat_amd/build.py's _units(()) is compiled device-only
with the build's own flags plus --cuda-device-only -fuse-cuid=none (without
the latter the object carries an id hashed from the source path, so two
copies of one tree differ).  A host-side refactor leaves every hash as it
was.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dragonboat_amd import build as B  # noqa: E402


def _hash(args):
    tmp, (name, src, defs, _) = args
    obj = os.path.join(tmp, name)
    subprocess.check_call(
        [B.HIPCC] + B.FLAGS + ["--cuda-device-only", "-fuse-cuid=none", "-c",
                               "-o", obj] + ["-D" + d for d in defs] +
        [os.path.join(B.CSRC, src)])
    with open(obj, "rb") as f:
        return name, hashlib.sha256(f.read()).hexdigest()


def main(argv):
    if len(argv) == 2:
        a, b = (json.load(open(p)) for p in argv)
        diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        print("%d of %d identical" % (len(a) - len(diff), len(a)))
        for k in diff:
            print("differs:", k)
        return 1 if diff or len(a) != len(b) else 0
    jobs = int(os.environ.get("DRB_BUILD_JOBS", 0)) or \
        max(1, min(16, os.cpu_count() or 1))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(jobs) as ex:
        out = dict(ex.map(_hash, [(tmp, u) for u in B._units(())]))
    with open(argv[0], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("%d units hashed" % len(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
