"""The bits of the retired kernel variants (the (chunk, tap) step loop of the 3x3 convolutions; the gather form of the stem's
un-pooling and the class form of its 7x7 input gradient), recorded in tests/golden/retired_variant_bits.json on the last
commit that had them.  The kernels that replaced them gave the same bits on every recorded case then, and are held to the
record now: a case's operands are rebuilt from their seeds, their digest must be the recorded one (so a failure says which
side moved), and the output must have the recorded digest and the recorded count of non-zero elements.

A digest is the SHA-256 of the tensors' bytes (contiguous, row-major, as stored: bf16 as 2 bytes, fp32 as 4, uint8 as 1),
concatenated in the order the case lists them:
    adil_conv3x3            x, wp                          (wp' and g for the flipped rows)
    adil_conv3x3_s2_fwd     x, wp
    adil_conv3x3_s2_bwd     g, wp_bwd
    adil_stem_conv_bwd      gy, wb, inv_std as three fp32
    adil_stem_pool_bwd      g, idx, p, scale"""
import hashlib
import json
import os

import torch

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retired_variant_bits.json")
_records = None


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def describe(inputs, out):
    """The record of one case."""
    return dict(inputs=digest(inputs), output=digest([out]), shape=list(out.shape), dtype=str(out.dtype).replace("torch.", ""),
                nonzero=int((out != 0).sum()))


def recorded(case):
    global _records
    if _records is None:
        with open(PATH) as f:
            _records = json.load(f)["records"]
    assert case in _records, f"{case}: no such record"
    return _records[case]


def check(case, inputs, out):
    want, got = recorded(case), describe(inputs, out)
    assert got["inputs"] == want["inputs"], f"{case}: operands drifted (the inputs no longer have the recorded digest)"
    assert (got["shape"], got["dtype"]) == (want["shape"], want["dtype"]), (case, got["shape"], got["dtype"])
    assert got["nonzero"] == want["nonzero"], f"{case}: {got['nonzero']} non-zero elements, {want['nonzero']} recorded"
    assert got["output"] == want["output"], f"{case}: the output's bits are not the recorded ones"
    return want
