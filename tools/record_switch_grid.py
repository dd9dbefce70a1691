"""Record what `zoo.build_classifier` does with its kernel switches: tests/golden/classifier_switch_grid.json.

For every case of the grid below (network x dtype x channels_last x a set of switches, all on the CPU with 8 classes) the
record holds either the exception's type and message or a census of the built model.  The record is made ONCE, on the
commit whose behaviour is to be kept, and replayed by tests/test_classifier_switches_cpu.py on every later one; this file
uses the public `build_classifier` alone, so it runs on any commit.

    python tools/record_switch_grid.py            # writes the record
    python tools/record_switch_grid.py --count    # prints how many cases the grid has, builds nothing

A case's key is "<network> <fp32|bf16> <nchw|cl> <switch>=<value>,...", switches in the order of KEYWORDS, values 1 or
"inference".  The census of a built model is the SHA-256 of the JSON of
    [len(model), [(qualified name, class name) of every module], [state-dict keys],
     [(name, dtype, shape, persistent) of every buffer], [(module name, attribute, value) of the attributes in ATTRS]]
stored with the count of modules per class, which is what a failing replay prints first."""
import argparse
import collections
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "classifier_switch_grid.json")

NETWORKS = ("resnet18", "resnet50", "mobilenet_v2", "densenet121", "vit_b_16", "vgg11")
RESNET_KEYWORDS = ("fuse_bn_act", "fuse_stem", "head_fp32", "own_strided_conv")
OWN_ROWS = {"mobilenet_v2": ("own_depthwise", "own_pointwise", "own_first_conv", "head_fp32"),
            "densenet121": ("own_dense_pointwise", "own_dense_conv", "own_dense_block", "own_dense_transition",
                            "own_dense_stem", "own_dense_head"),
            "vit_b_16": ("own_attention",)}
THREE_STATE = ("head_fp32", "own_dense_head")
KEYWORDS = ("fuse_bn_act", "fuse_stem", "own_strided_conv", "own_depthwise", "own_pointwise", "own_first_conv",
            "own_dense_pointwise", "own_dense_conv", "own_dense_block", "own_dense_transition", "own_dense_stem", "head_fp32",
            "own_dense_head", "own_attention")
ATTRS = ("head32_on", "pool_first", "own_attention", "own_strided_conv")
# a built ViT-B/16 or VGG11 costs most of a second: their successful cases are kept for these switch counts only
# (every error case and every other network's case is kept)
THIN = {"vit_b_16": (0, 1), "vgg11": (0, 1)}


def values_of(keyword):
    return (True, "inference") if keyword in THREE_STATE else (True,)


def switch_sets(network):
    """The switch sets of one network, as dicts, without repeats: none, every switch alone, every pair, every subset of the
    network's own rows, every combination of the four ResNet keywords (for the ResNets)."""
    atoms = [(k, v) for k in KEYWORDS for v in values_of(k)]
    sets = [{}] + [dict([a]) for a in atoms]
    sets += [dict([a, b]) for a, b in itertools.combinations(atoms, 2) if a[0] != b[0]]
    subsets = [OWN_ROWS.get(network, ())] + ([RESNET_KEYWORDS] if network.startswith("resnet") else [])
    for rows in subsets:
        for choice in itertools.product(*[(False,) + values_of(k) for k in rows]):
            sets.append({k: v for k, v in zip(rows, choice) if v})
    seen, out = set(), []
    for s in sets:
        tag = switches_text(s)
        if tag not in seen:
            seen.add(tag)
            out.append(s)
    return out


def switches_text(switches):
    return ",".join(f"{k}={'inference' if switches[k] == 'inference' else 1}" for k in KEYWORDS if k in switches)


def cases():
    """(key, network, bf16, channels_last, switches) of the whole grid."""
    for network in NETWORKS:
        for bf16, cl in itertools.product((False, True), (False, True)):
            for s in switch_sets(network):
                key = f"{network} {'bf16' if bf16 else 'fp32'} {'cl' if cl else 'nchw'} {switches_text(s)}".rstrip()
                yield key, network, bf16, cl, s


def census(model):
    import torch.nn as nn
    assert isinstance(model, nn.Module)
    modules = [(name, type(m).__name__) for name, m in model.named_modules()]
    buffers = [((prefix + "." if prefix else "") + name, str(b.dtype), list(b.shape), name not in m._non_persistent_buffers_set)
               for prefix, m in model.named_modules() for name, b in m.named_buffers(recurse=False)]
    attrs = [(name, a, m.__dict__[a] if a in m.__dict__ else getattr(type(m), a))
             for name, m in model.named_modules() for a in ATTRS if a in m.__dict__ or hasattr(type(m), a)]
    body = [len(model), modules, list(model.state_dict().keys()), buffers, attrs]
    sha = hashlib.sha256(json.dumps(body, sort_keys=True).encode()).hexdigest()
    return {"sha256": sha, "classes": dict(sorted(collections.Counter(c for _, c in modules).items()))}


def outcome(network, bf16, cl, switches):
    """{"error": [type, message]} or the census of the model `build_classifier` gives."""
    import torch
    from dl_attack_on_imagenet_amd import zoo
    try:
        model = zoo.build_classifier(network, num_classes=8, dtype=torch.bfloat16 if bf16 else torch.float32,
                                     channels_last=cl, **switches)
    except Exception as e:                                    # whatever it raises is the record
        return {"error": [type(e).__name__, str(e)]}
    return census(model)


def record():
    """The whole grid: {"outcomes": [unique outcomes], "cases": {key: index into outcomes}}."""
    outcomes, index, out = [], {}, {}
    for key, network, bf16, cl, switches in cases():
        got = outcome(network, bf16, cl, switches)
        if "error" not in got and network in THIN and len(switches) not in THIN[network]:
            continue
        tag = json.dumps(got, sort_keys=True)
        if tag not in index:
            index[tag] = len(outcomes)
            outcomes.append(got)
        out[key] = index[tag]
    return {"outcomes": outcomes, "cases": out}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--count", action="store_true", help="print the number of cases and stop")
    ap.add_argument("--out", default=PATH)
    a = ap.parse_args()
    if a.count:
        print(sum(1 for _ in cases()))
        sys.exit(0)
    sys.path.insert(0, ROOT)
    rec = record()
    with open(a.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    built = sum("error" not in rec["outcomes"][i] for i in rec["cases"].values())
    print(f"{len(rec['cases'])} cases ({built} built, {len(rec['outcomes'])} distinct outcomes) -> {a.out}")
