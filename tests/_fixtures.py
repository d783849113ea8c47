"""Stored reference outputs (``tests/fixtures/*.safetensors``,
``tests/golden/*.safetensors``) for the parity tests.  They were produced once
by ``scripts/gen_ref_fixtures.py`` from the reference's own sources; tests only
read tensors here, nothing of the reference is imported or executed in a test
process.  A set too large for one file is stored under ``tests/golden/`` in
parts, ``<name>.<part>.safetensors``, with disjoint keys."""
import functools
import glob
import os

from safetensors.torch import load_file

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def load(name: str) -> dict:
    whole = os.path.join(DIR, name + ".safetensors")
    if os.path.exists(whole):
        return load_file(whole)
    parts = sorted(glob.glob(os.path.join(GOLDEN, name + ".*.safetensors")))
    assert parts, f"no fixture {name!r} under {DIR} or {GOLDEN}"
    d = {}
    for p in parts:
        d.update(load_file(p))
    return d


def case(name: str, key: str):
    """All tensors of one case, ``{"in0": ..., "loss": ..., "grad0": ...}``."""
    d = load(name)
    p = key + "/"
    return {k[len(p):]: v.clone() for k, v in d.items() if k.startswith(p)}
