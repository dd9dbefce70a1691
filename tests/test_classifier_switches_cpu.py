"""CPU: `zoo.build_classifier` and the two CLIs are driven by one table of kernel switches (`zoo.SWITCHES`).

The grid of tests/golden/classifier_switch_grid.json (tools/record_switch_grid.py; recorded on the last commit that
checked and applied every switch by hand) is replayed: a case that raised must raise the same type with the same text in
front of the first " (", a case that built must give the same census (modules, state-dict keys, buffers with dtype, shape
and persistence, the switch attributes).  The CLI half checks the flags of every row and the argument-to-keyword rules
against a restatement written out here."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_switch_grid", os.path.join(ROOT, "tools", "record_switch_grid.py"))
grid = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(grid)

OFF = dict(own_depthwise=False, own_pointwise=False, own_first_conv=False, own_dense_pointwise=False, own_dense_conv=False,
           own_dense_block=False, own_dense_transition=False, own_dense_stem=False, head_fp32=False, own_dense_head=False,
           own_attention=False)
DENSE_FIVE = ("own_dense_pointwise", "own_dense_conv", "own_dense_block", "own_dense_transition", "own_dense_stem")


@pytest.fixture(scope="module")
def record():
    with open(grid.PATH) as f:
        return json.load(f)


def test_the_record_covers_the_grid(record):
    """Every case of the grid is in the record, but for the thinned successful ViT-B/16 / VGG11 ones; both kinds of
    outcome occur for every network."""
    keys = {key: (network, len(switches)) for key, network, _, _, switches in grid.cases()}
    assert set(record["cases"]) <= set(keys)
    for key in set(keys) - set(record["cases"]):
        network, n = keys[key]
        assert network in grid.THIN and n not in grid.THIN[network], key
    for network in grid.NETWORKS:
        kinds = {"error" in record["outcomes"][i] for key, i in record["cases"].items() if keys[key][0] == network}
        assert kinds == {False, True}, network


@pytest.mark.parametrize("network", grid.NETWORKS)
def test_replay(record, network):
    mine = [(key, bf16, cl, s) for key, net, bf16, cl, s in grid.cases() if net == network and key in record["cases"]]
    assert len(mine) > 500
    for key, bf16, cl, switches in mine:
        want, got = record["outcomes"][record["cases"][key]], grid.outcome(network, bf16, cl, switches)
        if "error" in want:
            assert "error" in got, f"{key}: built, recorded {want['error']}"
            assert got["error"][0] == want["error"][0], (key, got["error"], want["error"])
            assert got["error"][1].split(" (")[0] == want["error"][1].split(" (")[0], (key, got["error"], want["error"])
        else:
            assert "error" not in got, f"{key}: {got.get('error')}, recorded a built model"
            assert got["classes"] == want["classes"], key
            assert got["sha256"] == want["sha256"], f"{key}: same module classes, another census"


def test_bad_values_of_the_three_state_switches_are_refused_first():
    from dl_attack_on_imagenet_amd import zoo
    for kw in ("head_fp32", "own_dense_head"):
        with pytest.raises(ValueError, match=f"{kw} must be False, True or 'inference'"):
            zoo.build_classifier("vgg11", num_classes=8, **{kw: "always"})


def test_the_table_is_the_signature():
    """Every row is a keyword of build_classifier that defaults to off, in the table's order; a row's requirements come
    in front of it."""
    import inspect
    from dl_attack_on_imagenet_amd import zoo
    params = inspect.signature(zoo.build_classifier).parameters
    assert [r.keyword for r in zoo.SWITCHES] == list(OFF)
    for i, row in enumerate(zoo.SWITCHES):
        assert params[row.keyword].default is False
        assert set(row.requires) <= {r.keyword for r in zoo.SWITCHES[:i]}
        assert row.network in zoo.NETWORK_LABELS and row.dest == row.flag[2:].replace("-", "_")
    for row in zoo.SWITCHES:
        assert row.keyword in zoo.build_classifier.__doc__ and row.help in zoo.build_classifier.__doc__


def test_cli_flags_exist_default_to_off_and_refuse_other_values(capsys):
    import demo_dL_attack
    import main
    from dl_attack_on_imagenet_amd import zoo
    dense = [r for r in zoo.SWITCHES if r.keyword in DENSE_FIVE]
    assert len(dense) == 5 and tuple(main.DENSE_ROWS) == tuple(dense)
    for mod, rows in ((demo_dL_attack, zoo.SWITCHES), (main, dense)):
        p = mod.build_parser()
        off = p.parse_args([])
        for row in rows:
            on, bad = (("inference", "always"), "1") if row.three_state else ((1,), "2")
            assert getattr(off, row.dest) == ("0" if row.three_state else 0)
            for v in on:
                assert getattr(p.parse_args([row.flag, str(v)]), row.dest) == v
            with pytest.raises(SystemExit):
                p.parse_args([row.flag, bad])
            assert row.help in " ".join(p.format_help().split())
    capsys.readouterr()
    with pytest.raises(SystemExit):                                      # the head switches are not main.py's
        main.build_parser().parse_args(["--own-dense-head", "always"])


def _demo(argv):
    import demo_dL_attack
    args = demo_dL_attack.build_parser().parse_args(argv)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    return demo_dL_attack.classifier_keywords(args, args.model.lower(), dtype)


NOT_FAST = dict(fuse_bn_act=False, fuse_stem=False, own_strided_conv=False)


def test_demo_arguments_to_keywords():
    three = ["--own-dense-pointwise", "1", "--own-dense-conv", "1", "--own-dense-block", "1"]
    assert _demo(["-m", "densenet", "--dtype", "bf16"] + three) == dict(
        OFF, own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True, channels_last=True, **NOT_FAST)
    assert _demo(["-m", "densenet", "--dtype", "fp32"] + three) == dict(OFF, channels_last=False, **NOT_FAST)
    assert _demo(["-m", "mobilenet", "--dtype", "bf16"] + three) == dict(OFF, channels_last=False, **NOT_FAST)
    assert _demo(["-m", "mobilenet", "--dtype", "bf16", "--own-head", "inference"]) == dict(
        OFF, head_fp32="inference", channels_last=True, **NOT_FAST)
    assert _demo(["-m", "mobilenet", "--dtype", "bf16", "--own-head", "always"])["head_fp32"] is True
    assert _demo(["-m", "vit", "--dtype", "bf16", "--own-attention", "1"]) == dict(
        OFF, own_attention=True, channels_last=False, **NOT_FAST)
    fast = dict(OFF, head_fp32="inference", channels_last=True, fuse_bn_act=True, fuse_stem=True, own_strided_conv=False)
    assert _demo(["-m", "resnet50", "--dtype", "bf16"]) == fast
    assert _demo(["-m", "resnet50", "--dtype", "bf16", "--own-head", "always"]) == fast
    assert _demo(["-m", "resnet50", "--dtype", "bf16", "--own-strided-conv", "1"]) == dict(fast, own_strided_conv=True)
    assert _demo(["-m", "resnet50", "--dtype", "bf16", "--fast-classifier", "0", "--own-strided-conv", "1"]) == dict(
        OFF, channels_last=False, **NOT_FAST)
    # every row alone, on its own network in bf16: on, and channels_last exactly where the row needs it
    from dl_attack_on_imagenet_amd import zoo
    for row in zoo.SWITCHES:
        value = "always" if row.three_state else "1"
        got = _demo(["-m", row.network, "--dtype", "bf16", row.flag, value])
        assert got == dict(OFF, channels_last=row.channels_last, **NOT_FAST, **{row.keyword: True}), row.keyword


def test_main_arguments_to_keywords(monkeypatch):
    """main.py: the gate is the network alone; any active switch gives a bf16 channels_last network and a bf16 stream."""
    import main
    from dl_attack_on_imagenet_amd import zoo
    calls = []

    class Stop(Exception):
        pass

    def build(name, **kw):
        calls.append((name, kw))
        raise Stop

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: None)
    monkeypatch.setattr(zoo, "build_classifier", build)
    for argv in (["-m", "densenet", "--own-dense-stem", "1"], ["-m", "mobilenet", "--own-dense-stem", "1"]):
        with pytest.raises(Stop):
            main.main(main.build_parser().parse_args(argv))
    device = torch.device("cuda", 0)
    assert calls[0] == ("densenet", dict(weights=None, device=device, dtype=torch.bfloat16, channels_last=True,
                                         own_dense_pointwise=False, own_dense_conv=False, own_dense_block=False,
                                         own_dense_transition=False, own_dense_stem=True))
    assert calls[1] == ("mobilenet", dict(weights=None, device=device))              # the plain fp32 call
