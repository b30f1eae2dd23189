"""CPU: which kernel each max-pool call gets.  The selection (opental_amd/csrc/pool_select.h) is compiled with g++ through
tests/cpu_pool_select.cpp and asked about every pool item of tests/test_layer_calls_gpu.py: the recorded rows of the model's
workloads, their variants, the shapes the model never runs and the documented refusals.  The expected answers
(tests/golden/pool_choice.npz, written by tools/record_layer_calls.py pool_choice) are what the library reported on the GPU
for each of those calls BEFORE the selection moved into pool_select.h: return code and otal_layer_last_kernel().  The harness
serves the options' table defaults whatever the environment sets."""
import os

import numpy as np
import pytest

import pool_select_harness as PS
from oracle import layer_ref as R

SWITCHES = ("OTAL_POOL_NO133", "OTAL_POOL_NOROWS")


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return PS.build(tmp_path_factory.mktemp("cpupoolselect"))


@pytest.fixture(scope="module")
def Z(golden_dir):
    return np.load(os.path.join(golden_dir, "pool_choice.npz"))


def switches_of(Z, i):
    return tuple(s for s in str(Z["switches"][i]).split(",") if s)


def ask(H, Z, i, switches=None, ints=None):
    return PS.choose(H, str(Z["family"][i]), Z["ints"][i] if ints is None else ints, Z["addr16"][i],
                     switches_of(Z, i) if switches is None else switches)


def test_every_item_gets_its_recorded_kernel(H, Z):
    n = len(Z["label"])
    assert n > 300 and set(Z["family"]) == {"pool_fwd", "pool_bwd"}
    bad = []
    for i in range(n):
        c = ask(H, Z, i)
        if (c["rc"], c["kernel"]) != (int(Z["rc"][i]), str(Z["kernel"][i])):
            bad.append((str(Z["label"][i]), (c["rc"], c["kernel"]), (int(Z["rc"][i]), str(Z["kernel"][i]))))
    assert not bad, f"{len(bad)} of {n} items changed kernels, first: {bad[:5]}"


def test_every_kernel_is_in_the_fixture(H, Z):
    names = PS.kernel_names(H)
    assert len(names) == len(set(names)) and "?" not in names
    recorded = set(Z["kernel"].tolist()) - {""}
    assert recorded == set(names), (sorted(set(names) - recorded), sorted(recorded - set(names)))
    assert set(Z["rc"].tolist()) == {0, -7} and all((k == "") == (rc != 0) for k, rc in zip(Z["kernel"], Z["rc"]))


def test_the_batch_does_not_change_the_kernel(H, Z, golden_dir):
    """The GPU test clips B to 2; the rows as the model makes them (tests/golden/layer_calls.npz) choose the same kernel."""
    full = np.load(os.path.join(golden_dir, "layer_calls.npz"))
    seen = 0
    for i in range(len(Z["label"])):
        r = int(Z["row"][i])
        if r < 0 or str(Z["label"][i]).count("-") != str(full["source"][r]).count("-") + 2:      # base items only: no variant
            continue
        fam = R.FAMILY[str(full["entry"][r])]
        ints = full["ints"][r][:len(R.FIELDS[fam])]
        assert fam == str(Z["family"][i]) and ints[1:].tolist() == Z["ints"][i][1:len(ints)].tolist(), str(Z["label"][i])
        c = PS.choose(H, fam, ints, full["addr16"][r])
        assert (c["rc"], c["kernel"]) == (int(Z["rc"][i]), str(Z["kernel"][i])), (str(Z["label"][i]), c)
        assert c["gy"] == int(ints[0]) * int(ints[1])
        seen += int(ints[0] > 2)
    assert seen > 20


def test_the_switches_move_exactly_their_rows(H, Z):
    """OTAL_POOL_NO133 / OTAL_POOL_NOROWS change the answer for exactly the base rows whose -no133 / -norows twin in the
    fixture was served differently, and to that twin's answer; afterwards every answer is back."""
    label = [str(v) for v in Z["label"]]
    at = {l: i for i, l in enumerate(label)}
    plain = [i for i in range(len(label)) if not switches_of(Z, i)]
    for sw, suffix in zip(SWITCHES, ("-no133", "-norows")):
        twins = {l[:-len(suffix)]: i for l, i in at.items() if l.endswith(suffix)}
        assert len(twins) >= 4 and all(switches_of(Z, i) == (sw,) and b in at for b, i in twins.items())
        moved = {b for b, i in twins.items() if (int(Z["rc"][i]), str(Z["kernel"][i])) != (int(Z["rc"][at[b]]), str(Z["kernel"][at[b]]))}
        assert moved
        for i in plain:
            off, on = ask(H, Z, i), ask(H, Z, i, switches=(sw,))
            if label[i] in twins:
                t = twins[label[i]]
                assert (on["rc"], on["kernel"]) == (int(Z["rc"][t]), str(Z["kernel"][t])), (label[i], sw, on)
                assert ((on["rc"], on["kernel"]) != (off["rc"], off["kernel"])) == (label[i] in moved), (label[i], sw)
            again = ask(H, Z, i)
            assert again == off and (off["rc"], off["kernel"]) == (int(Z["rc"][i]), str(Z["kernel"][i])), (label[i], sw)


def lds_layout(kernel, d, c):
    """Bytes the kernel carves out of its dynamic LDS (pool3d.hip: the `sm` pointers of each kernel) for the planes per block
    of the same choice; None: the kernel has no dynamic LDS."""
    P, n = d["Hi"], c["planes"]
    if kernel.startswith("maxpool333_sep_fwd"):         # xs [n+2][Q][Q], rm [n+2][Q][P] floats; tw [n+2][Q][P], th [n+2][P][P] bytes
        Q = P + 2
        return (n + 2) * (Q * Q + Q * P) * 4 + (n + 2) * (Q * P + P * P)
    if kernel.startswith("maxpool333_rows_fwd"):        # srm, spm: [n+2][P][P] floats each
        return 2 * (n + 2) * P * P * 4
    if kernel.startswith("maxpool333_sep_bwd"):         # dys [n+2][PP], gp [n][PP], gr [n][PP] floats; tp [n+2][PP] bytes
        return ((n + 2) + 2 * n) * P * P * 4 + (n + 2) * P * P
    if kernel.startswith("maxpool333_rows_bwd"):        # sdy, sgp: [n+2][P][P] floats each; stp [(n+2)*P] tap rows of pitch TB
        return 2 * (n + 2) * P * P * 4 + (n + 2) * P * (P if P % 4 == 0 else 8)
    if kernel.startswith("maxpool3d_fwd_lds"):          # sm [(n-1)*st + kt][HL][WL] floats
        HL, WL = (d["Ho"] - 1) * d["sh"] + d["kh"], (d["Wo"] - 1) * d["sw"] + d["kw"]
        return ((n - 1) * d["st"] + d["kt"]) * HL * WL * 4
    if kernel.startswith("maxpool3d_bwd_lds"):          # sm [tlo_max][HLo][WLo] floats, sa: as many bytes (+ 16 of slack)
        ch, cw = -(-d["kh"] // d["sh"]), -(-d["kw"] // d["sw"])
        HLo, WLo = (d["Hi"] - 1 + d["ph"]) // d["sh"] + ch, (d["Wi"] - 1 + d["pw"]) // d["sw"] + cw
        return c["tlo_max"] * HLo * WLo * 5 + 16
    return None


def test_launch_bounds(H, Z):
    budget = int(H.cpu_pool_lds_budget())
    assert budget == 48 * 1024
    with_lds = set()
    for i in range(len(Z["label"])):
        c = ask(H, Z, i)
        if c["rc"]:
            continue
        fam, k, label = str(Z["family"][i]), c["kernel"], str(Z["label"][i])
        d = R.unpack(fam, Z["ints"][i])
        assert c["gx"] >= 1 and c["gy"] == d["B"] * d["C"] <= 65535, (label, c)
        want = lds_layout(k, d, c)
        assert c["lds"] == (want or 0), (label, c, want)
        if want is not None:
            with_lds.add(k.split("<")[0])
            assert c["planes"] >= 1
        if k.startswith(("maxpool3d_fwd_lds", "maxpool3d_bwd_lds", "maxpool333_sep_fwd")):
            assert c["lds"] <= budget, (label, c)
        # the planes of all blocks cover the map along T
        if want is not None:
            assert c["gx"] == -(-d["Ti" if fam == "pool_bwd" else "To"] // c["planes"]), (label, c)
    assert with_lds == {"maxpool333_sep_fwd", "maxpool333_rows_fwd", "maxpool333_sep_bwd", "maxpool333_rows_bwd",
                        "maxpool3d_fwd_lds", "maxpool3d_bwd_lds"}
