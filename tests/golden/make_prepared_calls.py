#!/usr/bin/env python
"""Freeze what a prepared call is: ``tests/golden/prepared_calls.json`` (the rows of ``tests/prepared_rows.py``).

    PYTHONPATH=<a checkout of the commit to freeze> python tests/golden/make_prepared_calls.py [OUT]

Needs no GPU: every call is prepared with ``launch=False`` on CPU tensors.  The ``chemprop_amd`` that is frozen is the first one on
``sys.path`` — a checkout of the PARENT of a refactoring commit on ``PYTHONPATH`` (with its library built), never the refactored code:
the file is what holds the refactoring to the behaviour before it.  Without ``PYTHONPATH`` it freezes this tree.  ``OUT``: another
path to write to (the file must come out the same on a machine with and without a GPU: write a second copy there and compare).
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/: the row builder
sys.path.append(os.path.dirname(os.path.dirname(HERE)))       # this tree LAST: a checkout on PYTHONPATH comes first

import prepared_rows  # noqa: E402
from chemprop_amd import engine  # noqa: E402


def main():
    engine._require_device = lambda t, name: None   # (CPU tensors: nothing is launched)
    rows = prepared_rows.build_rows()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "prepared_calls.json")
    with open(path, "w") as f:
        f.write(prepared_rows.dumps(rows))
    print(f"{len(rows)} rows of {os.path.dirname(engine.__file__)} -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
