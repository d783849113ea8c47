"""Conv routing is pinned: ``mda_conv_route`` (the planner of
csrc/conv_igemm.hip, run dry through the real entry points) must choose, for
every shape in ``tests/golden/conv_routes.json``, exactly the kernel, tile,
grid, K-steps, splits and status that the launch code of commit 914f1b4
launched.  The fixture was recorded from that commit's host layer with its
launches replaced by a recorder; for ``mda_conv_fwd_bnstats`` it also holds the
per-block partial-row count ``nblk`` that commit computed by hand.  Host code
only: no GPU."""
import json
import os
import shutil

import pytest
import torch

from mdistiller_ddp_amd.ops import _ext

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "conv_routes.json")

pytestmark = pytest.mark.skipif(
    not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc") or os.environ.get("HIPCC")),
    reason="hipcc absent: the native library cannot be built")


def test_routes_match_recorded_parent():
    _ext.load(required=True)
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["shape_fields"][0] == "op" and len(fx["shape_fields"]) == 17
    fields = fx["route_fields"]
    assert len(fx["cases"]) >= 1000
    out = torch.zeros(len(fields), dtype=torch.int64)
    bad = []
    for note, shape, want in fx["cases"]:
        out.fill_(-7)
        _ext.call("mda_conv_route", *shape, out)
        got = out.tolist()
        if got != want:
            diff = {k: (g, w) for k, g, w in zip(fields, got, want) if g != w}
            bad.append((note, dict(zip(fx["shape_fields"], shape)), diff))
    assert not bad, f"{len(bad)} of {len(fx['cases'])} routes differ (got, want); first: {bad[:5]}"


def test_fixture_covers_every_path():
    """The recorded cases reach every kernel family, ring, flip, load mode, tile,
    the streaming-1x1 offer, split-K, both error statuses and all five ops."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    i = {k: n for n, k in enumerate(fx["route_fields"])}
    ok = [r for _, _, r in fx["cases"] if r[i["rc"]] == 0]
    assert {s[0] for _, s, _ in fx["cases"]} == {0, 1, 2, 3, 4}
    assert {r[i["rc"]] for _, _, r in fx["cases"]} == {0, 1, _ext.NOT_SERVED}
    assert {(r[i["family"]], r[i["ring"]]) for r in ok} == {(0, 1), (0, 3), (1, 0), (2, 3), (3, 0)}
    assert {(r[i["family"]], r[i["flip"]]) for r in ok if r[i["family"]] >= 2} == {(2, 0), (2, 1), (3, 0), (3, 1)}
    assert {r[i["mode"]] for r in ok} == {0, 1, 2, 3, 4}
    assert {(r[i["bm"]], r[i["bn"]]) for r in ok if r[i["family"]] < 2} == {
        (128, 128), (128, 64), (128, 32), (64, 128), (64, 64), (64, 32)}
    # grouped convs: ShuffleNetV1's group widths, forward (Cout / groups) and
    # dgrad (its GEMM's N is Cin / groups), through the grouped N-tile fit
    s = {k: n for n, k in enumerate(fx["shape_fields"])}
    served = [(sh, r) for _, sh, r in fx["cases"] if r[i["rc"]] == 0 and sh[s["groups"]] > 1]
    assert {sh[s["Cout"]] // sh[s["groups"]] for sh, _ in served if sh[0] == 2} >= {24, 72, 80, 160}
    assert {sh[s["Cin"]] // sh[s["groups"]] for sh, _ in served if sh[0] == 3} >= {24, 80, 160}
    notes = {note for note, _, _ in fx["cases"]}
    assert {"resnet32x4", "ShuffleV1"} <= notes  # layers read from the model definitions
    # an oversized 1x1 conv + BN statistics: no streaming offer when it would fuse
    over = [r for note, sh, r in fx["cases"] if sh[0] == 1 and note.startswith("error: 32-bit")]
    assert {(r[i["rc"]], r[i["stream1x1"]]) for r in over} == {(1, 0), (1, 1)}
    assert {r[i["stream1x1"]] for r in ok} == {0, 1}
    assert {r[i["splits"]] for r in ok} >= {1, 2, 4, 8}
