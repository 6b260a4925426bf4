"""Record the names tests/test_abi.py needs from the Go reference as tests/golden/reference_names.json.

The binding under go/ replaces four of the reference's files (sha1.go, sha1_efes.go, crc32.go,
crc32_efes.go) under `-tags efesgpu`.  The tests check it against WHAT those files define and what
the other files use of it -- names only, no source text:

  digest_files  {file: {"methods": [[type, name]...] with a receiver, "defined": package-level names}}
  other_files   {file: {"digest_methods": methods it defines on sha1digest / crc32digest (none),
                        "uses": the names of `defined` it mentions outside comments and strings}}
  build_lines   the 1-based lines of Makefile holding "CGO_ENABLED=0 go build" and of
                .goreleaser.yml holding "CGO_ENABLED=0" (INTEGRATION.md section 1 cites them)

Usage: python tests/golden/make_reference_names.py <checkout of the reference>
"""
from __future__ import annotations

import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_abi import DIGEST_FILES, _go_funcs  # noqa: E402


def main(ref: str) -> None:
    digest_files, defined = {}, set()
    for f in DIGEST_FILES:
        src = open(os.path.join(ref, f)).read()
        names = {n for r, _t, n, _ in _go_funcs(src) if not r}
        names |= set(re.findall(r"^(?:var|const|type) (\w+)", src, flags=re.M))
        for blk in re.findall(r"^(?:var|const) \((.*?)^\)", src, flags=re.M | re.S):
            names |= set(re.findall(r"^\s+(\w+)", blk, flags=re.M))
        digest_files[f] = {"methods": sorted([t, n] for r, t, n, _ in _go_funcs(src) if r), "defined": sorted(names)}
        defined |= names
    other_files = {}
    for f in sorted(os.listdir(ref)):
        if not f.endswith(".go") or f in DIGEST_FILES:
            continue
        src = open(os.path.join(ref, f)).read()
        src = re.sub(r'//.*$|"(?:\\.|[^"\\])*"|`[^`]*`', "", src, flags=re.M)  # code only
        other_files[f] = {
            "digest_methods": sorted([t, n] for r, t, n, _ in _go_funcs(src) if r and t in ("sha1digest", "crc32digest")),
            "uses": sorted(n for n in defined if re.search(rf"(?<![.\w]){n}\b", src))}

    def lines_with(name: str, text: str) -> list:
        return [i + 1 for i, line in enumerate(open(os.path.join(ref, name)).read().split("\n")) if text in line]

    out = {"digest_files": digest_files, "other_files": other_files,
           "build_lines": {"Makefile": lines_with("Makefile", "CGO_ENABLED=0 go build"),
                           ".goreleaser.yml": lines_with(".goreleaser.yml", "CGO_ENABLED=0")}}
    with open(os.path.join(HERE, "reference_names.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote reference_names.json")


if __name__ == "__main__":
    main(sys.argv[1])
