"""Mesh files of the reference tree kept unchanged in tests/golden.  tests/golden/reference_files.json maps each file's path in the reference
tree to its copy here and to the sha256 of the original, so the tests that check a copy against the shipped file need no reference tree."""
import hashlib
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "reference_files.json")))


def reference_file(rel):
    """path of the copy of `rel` (a path in the reference tree); asserts that the copy is byte-identical to the original"""
    entry = MANIFEST[rel]
    path = os.path.join(GOLDEN, entry["golden"])
    with open(path, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == entry["sha256"], "%s is not the reference's %s" % (path, rel)
    return path
