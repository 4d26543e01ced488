"""The states the weight-pack tests share: the whole-model cases of tests/test_gpu_pack.py with their edge state,
and the cases whose host-pack bytes tests/golden/pack_digests.json pins (tests/test_pack_host_bytes.py,
tests/golden/gen_pack_digests.py)."""
import hashlib

import numpy as np

import headset_cases as hc
from sfa_hip import _lib, runtime, synthetic

CASES = {
    "five": ("fpn_resnet_18", dict(runtime.DEFAULT_HEADS)),
    "two": ("fpn_resnet_18", hc.SETS["two"]),
    "eight_full": ("fpn_resnet_18", hc.SETS["eight_full"]),
    "resnet_18": ("resnet_18", dict(runtime.DEFAULT_HEADS)),
}
FAMILIES = ("fpn_resnet_18", "resnet_18")
DIGEST_SEEDS = (0, 2)


def edge_state(arch, seed=11):
    """synthetic_state_dict with rows replaced so that each rule of the pack is exercised (finite, normal)."""
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), seed)
    below = np.nextafter(np.float32(0.125), np.float32(0))
    w = sd["layer1.0.conv1.weight"]  # BN-folded 3x3 rows
    w[0] = 0  # an all-zero output row: e stays 13
    sd["layer1.0.bn1.weight"][1] = -abs(sd["layer1.0.bn1.weight"][1]) - 0.5  # a negative gamma
    sd["layer1.0.bn1.running_var"][2] = 0  # var = 0: scale = gamma / sqrt(1e-5)
    w[3] *= np.float32(2.0 ** -20)  # entries 2^-20 of the row maximum: fp16 low terms subnormal or zero
    w[3, 0, 0, 0] = 0.75
    f = sd["conv_up_level1.weight"] if "conv_up_level1.weight" in sd else None
    names = [n for n in sd if n.endswith(".0.weight") and "downsample" not in n and "deconv" not in n]  # heads' 3x3 convs
    h = sd[names[0]]
    for t in ([f, h] if f is not None else [h]):
        t[0] = np.clip(t[0], -0.1, 0.1)
        t[0].flat[0] = 0.125  # row maximum exactly 2^-3
        t[1] = np.clip(t[1], -0.1, 0.1)
        t[1].flat[1] = -below  # ... and the float below it
        t[2] *= np.float32(2.0 ** -20)
        t[2].flat[2] = 0.5
    # a downsample block whose two shifts cancel to near zero: sh(bn2) = -sh(downsample.1) up to rounding
    p = "layer2.0."
    sd[p + "bn2.running_mean"][:] = 0
    sd[p + "downsample.1.running_mean"][:] = 0
    sd[p + "downsample.1.bias"][:] = -sd[p + "bn2.bias"]
    sd[p + "downsample.1.bias"][0] = np.nextafter(sd[p + "downsample.1.bias"][0], np.float32(1))
    # biases of -0.0: a plain head bias, a w1 bias and a BatchNorm shift
    sd[names[0].replace(".0.weight", ".0.bias")][5] = np.float32(-0.0)
    sd[names[0].replace(".0.weight", ".2.bias")][0] = np.float32(-0.0)
    sd["bn1.bias"][7] = np.float32(-0.0)
    sd["bn1.running_mean"][7] = 0
    return sd


def digest_cases():
    """{case id: (arch descriptor, state builder)}: edge_state for each of CASES, synthetic_state_dict for
    DIGEST_SEEDS over every set of headset_cases.SETS in both families."""
    out = {}
    for name, (family, heads) in CASES.items():
        arch = hc.make_arch(heads, family)
        out[f"edge/{name}"] = (arch, lambda arch=arch: edge_state(arch))
    for family in FAMILIES:
        for name, heads in hc.SETS.items():
            arch = hc.make_arch(heads, family)
            for seed in DIGEST_SEEDS:
                out[f"synthetic/{family}/{name}/seed{seed}"] = (
                    arch, lambda arch=arch, seed=seed: synthetic.synthetic_state_dict(_lib.state_layout(arch), seed))
    return out


def digests(arch, sd):
    """(sha256 of the state's float32 bytes in layout order, the counters left out; sha256 of the host pack)."""
    h = hashlib.sha256()
    for name, _ in _lib.state_layout(arch):
        if not name.endswith("num_batches_tracked"):
            h.update(np.ascontiguousarray(sd[name], np.float32).tobytes())
    packed = runtime.pack_state_dict(sd, arch)
    return h.hexdigest(), hashlib.sha256(packed.view(np.uint8)).hexdigest()
