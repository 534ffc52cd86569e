#!/usr/bin/env python3
"""Records what tests/test_go_shim.py needs to know of the Handel reference,
as digests, in tests/golden/reference_go_digests.json, so the tests need no
reference tree:

  patch_preimage  per hunk of go/handel/config_hook.patch, "file:line:count" ->
                  SHA-256 of the `count` lines the reference file holds from
                  `line` on (the hunk applies there exactly when they are the
                  hunk's context and removed lines)
  identifiers     of the identifiers go/handel/batched_processing.go uses, the
                  ones the reference's package-handel sources (*.go in its
                  root) hold too: the first 12 hex digits of their SHA-256

Only digests are stored, none of the reference's text.

Usage: python tools/reference_digests.py REFERENCE_DIR
"""

from __future__ import annotations

import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO_HANDEL = os.path.join(ROOT, "go", "handel")
OUT = os.path.join(ROOT, "tests", "golden", "reference_go_digests.json")
IDENT = r"[A-Za-z_]\w*"


def digest(text: str) -> str:
    return hashlib.sha256(text.encode()).hexdigest()


def patch_hunks(path: str = os.path.join(GO_HANDEL, "config_hook.patch")):
    """[(file, first line, pre-image lines)] of a unified diff: per hunk the
    lines it expects in the file it patches (context and removed lines), with
    the line counts of its header checked against its body."""
    hunks, name, cur = [], None, None
    for ln in open(path).read().split("\n"):
        m = re.match(r"@@ -(\d+),(\d+) \+(\d+),(\d+) @@", ln)
        if ln.startswith("--- a/"):
            name, cur = ln[6:], None
        elif m and name:
            cur = {"file": name, "start": int(m.group(1)), "old": int(m.group(2)), "new": int(m.group(4)),
                   "pre": [], "post": 0}
            hunks.append(cur)
        elif cur is not None and ln[:1] in (" ", "-", "+") and not ln.startswith("+++ "):
            if ln[0] != "+":
                cur["pre"].append(ln[1:])
            if ln[0] != "-":
                cur["post"] += 1
    for h in hunks:
        assert len(h["pre"]) == h["old"] and h["post"] == h["new"], f"hunk header of {h['file']}:{h['start']}"
    return [(h["file"], h["start"], h["pre"]) for h in hunks]


def main(ref: str) -> None:
    pre = {}
    for f, start, lines in patch_hunks():
        have = open(os.path.join(ref, f)).read().split("\n")[start - 1:start - 1 + len(lines)]
        pre[f"{f}:{start}:{len(lines)}"] = digest("\n".join(have))
    theirs = set()
    for f in sorted(os.listdir(ref)):
        if f.endswith(".go"):
            theirs |= set(re.findall(IDENT, open(os.path.join(ref, f)).read()))
    ours = set(re.findall(IDENT, open(os.path.join(GO_HANDEL, "batched_processing.go")).read()))
    out = {"patch_preimage": pre, "identifiers": sorted(digest(n)[:12] for n in ours & theirs)}
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
