#!/usr/bin/env python3
"""Generates tests/golden/reference_tree.json: what the CPU tests need to know about the yahoo/bftkv tree the shim is written
against, so that they run without that tree.

  declared   for each name of tests/test_shim_static.py REFERENCE_NAMES the reference declares: the .go file that declares it
  hunks      for each hunk of shim/patches/*.patch, applied in order: the line the hunk starts at in the tree as the earlier
             patches left it, and the SHA-256 of the lines it replaces there (its context and removed lines, exactly)

No source text of the tree is stored.  Run with the root of the tree as the argument (or BFTKV_SRC in the environment) whenever a
patch or REFERENCE_NAMES changes.
"""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_tree.json")
sys.path.insert(0, ROOT)

from tests.test_shim_patches import parse_patch  # noqa: E402
from tests.test_shim_static import REFERENCE_NAMES, declaration_pattern  # noqa: E402


def main(src):
    declared = {}
    for dirpath, _, files in sorted(os.walk(src)):
        for f in sorted(files):
            if f.endswith(".go") and not f.endswith("_test.go"):
                p = os.path.join(dirpath, f)
                text = open(p, errors="replace").read()
                for name in REFERENCE_NAMES:
                    if name not in declared and re.search(declaration_pattern(name), text, flags=re.M):
                        declared[name] = os.path.relpath(p, src)
    trees, hunks = {}, {}
    pdir = os.path.join(ROOT, "shim", "patches")
    for name in sorted(f for f in os.listdir(pdir) if f.endswith(".patch")):
        hunks[name], shift = [], {}          # (a hunk's line numbers are those of the tree before its patch)
        for path, old_start, pre, post in parse_patch(open(os.path.join(pdir, name)).read()):
            if path not in trees:
                trees[path] = open(os.path.join(src, path)).read().splitlines(keepends=True)
            lines = trees[path]
            at = old_start - 1 + shift.get(path, 0)
            shift[path] = shift.get(path, 0) + len(post) - len(pre)
            assert lines[at:at + len(pre)] == pre, (name, path, old_start, "the hunk does not apply exactly where it says")
            hunks[name].append({"file": path, "line": old_start, "sha256": hashlib.sha256("".join(pre).encode()).hexdigest()})
            lines[at:at + len(pre)] = post
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/make_reference_tree.py", "declared": declared, "hunks": hunks}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["BFTKV_SRC"])
