"""CPU side of the head-set parity tests (tests/headset_cases.py, tests/test_gpu_headsets.py):

* the f32 oracle's forward of head sets other than the production one equals the reference's own forward
  (tests/golden/gen_headsets_golden.py), bit for bit as test_oracle_golden.py asks of the five-head model;
* the premises without which a wrong kernel could pass hold for every set on both batches, on the weights
  and the f64 oracle alone;
* the checker is sensitive: oracle data with a swapped, shifted, unwritten or misplaced channel fails
  stage_cases.failures in every group, at the gate and in the metric the GPU test uses;
* the descriptor's whole range packs; one head or one channel more is refused.
"""
import ctypes

import numpy as np
import pytest
import torch

import golden_io
import headset_cases as hc
import stage_cases as sc
from conftest import GOLDEN
from oracle import model_oracle as mo
from sfa_hip import _lib, runtime


@pytest.fixture(scope="module")
def fixture():
    return golden_io.load(GOLDEN, "headsets_golden")


@pytest.fixture(scope="module")
def up_levels():
    """batch -> {"x", "up_level2..4"}: the f64 oracle's backbone and neck, once per batch (synthetic weights
    are a function of the entry's name, so every set has the same backbone)."""
    sd64 = mo.state_dict_torch(hc.state_dict_np(hc.SETS["one"]), torch.float64)
    out = {}
    with torch.no_grad():
        for name, make in hc.BATCHES.items():
            x = torch.from_numpy(make())
            c = sc.run_stages(sd64, {"x": x}, {}, chain=True, only=("layer1", "layer2", "layer3", "layer4", "up_level2",
                                                                   "up_level3", "up_level4"))
            out[name] = {"x": x, **{k: c[k] for k in ("up_level2", "up_level3", "up_level4")}}
    return out


_REF = {}


def oracle_ref(up_levels, batch, name):
    """The f64 oracle's head maps and outputs of one set on one batch (shared, never modified)."""
    if (batch, name) not in _REF:
        heads = hc.SETS[name]
        sd64 = hc.head_state_f64(hc.state_dict_np(heads), heads)
        with torch.no_grad():
            _REF[batch, name] = (sd64, hc.oracle_heads_and_out(sd64, up_levels[batch], heads))
    return _REF[batch, name]


def test_sets_follow_the_rules():
    widths = {n: list(h.values()) for n, h in hc.SETS.items()}
    assert [64 * len(w) for w in widths.values()] == [64, 128, 192, 320, 320, 384, 512]
    assert all(1 <= c <= 4 for w in widths.values() for c in w)
    assert len(hc.SETS["eight_full"]) == _lib.SFA_MAX_HEADS and sum(widths["eight_full"]) == 32
    assert np.cumsum([0] + widths["five_wide"]).tolist() == [0, 4, 5, 9, 11, 15]
    assert widths["six"] == [3, 2, 2, 1, 3, 4] and set(widths["five_ones"]) == {1}
    for n in hc.UNSORTED:  # insertion order is not sorted() order, and heads that trade places differ in width
        h = hc.SETS[n]
        assert list(h) != sorted(h)
        moved = [(a, b) for a, b in zip(h, sorted(h)) if a != b]
        assert moved and any(h[a] != h[b] for a, b in moved), n


@pytest.mark.parametrize("arch,name", hc.FIXTURE_CASES)
def test_fixture_shapes_and_order(fixture, arch, name):
    heads = hc.SETS[name]
    assert [str(k) for k in fixture[f"{arch}/{name}/heads"]] == list(heads), "the reference emits insertion order"
    B, H, W, _ = hc.FIXTURE_INPUT
    for h, c in heads.items():
        assert fixture[f"{arch}/{name}/{h}"].shape == (B, c, H // 4, W // 4)


@pytest.mark.parametrize("name", [n for a, n in hc.FIXTURE_CASES if a == "fpn_resnet_18"])
def test_oracle_forward_matches_reference(fixture, name):
    """model_oracle.forward with one, five wide and eight heads == the reference's get_pose_net(18, heads, 64)
    on the same weights and input: the bound of test_oracle_golden.test_model_oracle_matches_reference."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    heads = hc.SETS[name]
    sd = mo.state_dict_torch(hc.state_dict_np(heads))
    with torch.no_grad():
        out = mo.forward(sd, torch.from_numpy(hc.fixture_input()), heads)
    assert list(out) == list(heads)
    for h in heads:
        np.testing.assert_array_equal(out[h].numpy(), fixture[f"fpn_resnet_18/{name}/{h}"], err_msg=h)


@pytest.mark.parametrize("arch", ["fpn_resnet_18", "resnet_18"])
@pytest.mark.parametrize("name", list(hc.SETS))
def test_weight_premises(name, arch):
    heads = hc.SETS[name]
    sd = hc.state_dict_np(heads, arch)
    hc.assert_weight_premises(sd, heads, arch)
    raw = hc.synthetic.synthetic_state_dict([(n, s) for n, s in _lib.state_layout(hc.make_arch(heads, arch))
                                             if n.endswith(".bias")], hc.WEIGHT_SEED)
    changed = [k for k in raw if not np.array_equal(raw[k], sd[k])]
    print(f"{arch} {name}: condition_biases changed {changed or 'nothing'}")


def test_condition_biases_repairs_zeros_and_repeats():
    heads = hc.SETS["two"]
    sd = hc.state_dict_np(heads)
    sd["fpn1_z_coor.0.bias"][7] = 0
    sd["fpn2_cen_offset.2.bias"][:] = sd["fpn0_cen_offset.2.bias"]
    with pytest.raises(AssertionError):
        hc.assert_weight_premises(sd, heads)
    assert hc.condition_biases(sd, heads) == 1 + 4
    hc.assert_weight_premises(sd, heads)


@pytest.mark.parametrize("batch", list(hc.BATCHES))
@pytest.mark.parametrize("name", list(hc.SETS))
def test_output_premises(up_levels, name, batch):
    heads = hc.SETS[name]
    sd64, ref = oracle_ref(up_levels, batch, name)
    hc.assert_output_premises(ref, heads, f"{name} {batch}")
    hc.assert_relu_live(sd64, up_levels[batch], heads, f"{name} {batch}")


def _rows(got, ref, heads):
    return sc.compare(got, ref, heads, per_frame=True)


@pytest.mark.parametrize("name", list(hc.SETS))
def test_checker_passes_clean_data(up_levels, name):
    """The oracle's own maps rounded to f32 pass: what fails below fails for the corruption alone."""
    heads = hc.SETS[name]
    _, ref = oracle_ref(up_levels, "3x64x96", name)
    got = {k: v.to(torch.float32) for k, v in ref.items()}
    assert not sc.failures(_rows(got, ref, heads))


def test_every_corruption_has_its_sets():
    """Each kind applies to the sets that can show it: the widest sets to all four."""
    on = {k: [n for n, h in hc.SETS.items() if hc.applies(k, h)] for k in hc.CORRUPTIONS}
    assert on["swap_channels"] == ["two", "three", "five_wide", "six", "eight_full"]
    assert on["shift_after_first"] == [n for n in hc.SETS if n != "one"]
    assert on["zero_channel_3"] == ["two", "five_wide", "six", "eight_full"]
    assert on["swap_heads"] == ["five_wide", "five_ones", "six", "eight_full"]


@pytest.mark.parametrize("name,kind", [(n, k) for n, h in hc.SETS.items() for k in hc.CORRUPTIONS if hc.applies(k, h)])
def test_checker_is_sensitive(up_levels, name, kind):
    """Two channels of a head swapped, every channel after the first head shifted by one, channel 3 of a
    4-channel head zero, two heads of equal width swapped: each is caught in every group."""
    heads = hc.SETS[name]
    _, ref = oracle_ref(up_levels, "3x64x96", name)
    bad = sc.failures(_rows(hc.corrupt(ref, heads, kind), ref, heads))
    assert bad
    for g in hc.GROUPS:
        assert any(b.startswith(g + "/") for b in bad), (g, bad)


@pytest.mark.parametrize("arch", ["fpn_resnet_18", "resnet_18"])
@pytest.mark.parametrize("name", list(hc.SETS))
def test_descriptor_range_packs(name, arch):
    """sfa_state_entry, sfa_packed_floats and sfa_pack_weights take every set; the heads are laid out in
    sorted() order in the state dict."""
    heads = hc.SETS[name]
    a = hc.make_arch(heads, arch)
    layout = _lib.state_layout(a)  # sfa_state_count + sfa_state_entry
    levels = 1 if arch == "resnet_18" else 3
    prefixes = {p for _, p in hc.head_prefixes(heads, arch)}
    head_entries = [n for n, _ in layout if n.rsplit(".", 2)[0] in prefixes]
    assert len(prefixes) == levels * len(heads) and len(head_entries) == 4 * len(prefixes)
    firsts = [n[:-len(".0.weight")] for n in head_entries if n.endswith(".0.weight")][:len(heads)]
    assert firsts == [("" if arch == "resnet_18" else "fpn0_") + h for h in sorted(heads)]
    shapes = dict(layout)
    for h, p in hc.head_prefixes(heads, arch):
        assert shapes[p + ".2.weight"] == (heads[h], 64, 1, 1) and shapes[p + ".2.bias"] == (heads[h],)
    n = int(_lib.arch_fn(a, "sfa_packed_floats")(ctypes.byref(a)))
    packed = runtime.pack_state_dict(hc.state_dict_np(heads, arch), a)
    assert n > 0 and packed.size == n and np.isfinite(packed).all()


def test_descriptor_refuses_a_ninth_head_and_a_fifth_channel():
    L = _lib.lib()
    nine = _lib.make_arch(hc.SETS["eight_full"])
    nine.num_heads = _lib.SFA_MAX_HEADS + 1
    five = _lib.make_arch({"hm_cen": 5})
    with pytest.raises(ValueError):
        _lib.make_arch({f"h{j}": 1 for j in range(9)})
    buf, shape, nd = ctypes.create_string_buffer(128), (ctypes.c_int64 * 4)(), ctypes.c_int()
    state = np.zeros(16, np.float32)
    for a in (nine, five):
        assert L.sfa_state_count(ctypes.byref(a)) == -1
        assert L.sfa_state_entry(ctypes.byref(a), 0, buf, 128, shape, ctypes.byref(nd)) != _lib.SFA_OK
        assert L.sfa_state_floats(ctypes.byref(a)) == 0
        assert L.sfa_packed_floats(ctypes.byref(a)) == 0
        assert L.sfa_pack_weights(ctypes.byref(a), state.ctypes.data, state.size, state.ctypes.data) != _lib.SFA_OK
        out = ctypes.c_void_p()
        assert L.sfa_model_create(ctypes.byref(a), state.ctypes.data, ctypes.byref(out)) != _lib.SFA_OK
        assert not out.value
