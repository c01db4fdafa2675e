"""CPU: the swap-consistency report's float64 twins (tests/swap_ref.py) against independent restatements, the mutants the GPU tests'
comparisons must reject, the argument checks of sv_swap_* that run before any launch, and the host side of split_vae_amd.swap (flags,
parser, refusals, the figures, the line).  No device work."""
import ctypes as C

import numpy as np
import pytest

import swap_ref as ref


@pytest.fixture(scope="module")
def lib(lib_built):
    from split_vae_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def lattice(lib):
    chunk = lib.sv_swap_chunk_rows()
    assert chunk >= 64 and chunk % 64 == 0
    cases = []
    for n, (Nq, Nr, L, _, _, _) in enumerate(ref.lattice_shapes(chunk)):
        c = ref.lattice_case(Nq, Nr, L, 100 + n)
        c["want"] = ref.rank(c["Q"], c["R"], c["t0"], c["t1"])
        cases.append(c)
    return cases


# ---------------------------------------------------------------- the twins
def test_rank_twin_equals_the_argsort_restatement_on_lattices_with_ties(lattice):
    ties = 0
    for c in lattice:
        assert ref.ranks_equal(c["want"], ref.rank_by_argsort(c["Q"], c["R"], c["t0"], c["t1"]))
        d = ref.distances(c["Q"], c["R"])
        ties += int(sum((d[q] == d[q, c["t0"][q]]).sum() - 1 for q in range(d.shape[0])))
        assert np.abs(c["Q"]).max() <= 4 and np.abs(c["R"]).max() <= 4 and (c["Q"] == np.rint(c["Q"])).all()
        assert d.max() < 2 ** 24                                           # every norm, dot product and distance is exact in fp32
    assert ties > 1000                                                     # ties are frequent
    spread = np.concatenate([c["want"].reshape(-1) for c in lattice])
    assert spread.min() == 0 and spread.max() > 1000 and len(np.unique(spread)) > 100


def test_lattice_cases_hold_the_named_situations(lattice, lib):
    chunk = lib.sv_swap_chunk_rows()
    shapes = ref.lattice_shapes(chunk)
    assert {s[0] for s in shapes} >= {1, 63, 64, 65, 130}
    assert {s[1] for s in shapes} >= {1, 2, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 3}
    assert {s[2] for s in shapes} >= {1, 3, 31, 32, 33, 128, 256}
    assert any(s[3] for s in shapes) and any(s[4] for s in shapes) and any(s[5] for s in shapes)
    c = lattice[4]
    Nr = c["R"].shape[0]
    assert c["t0"][0] == 0 and c["t1"][0] == Nr - 1 and c["t0"][1] == c["t1"][1]
    assert (c["Q"][2] == c["R"][c["t0"][2]]).all()                         # a query equal to its target
    mid = c["t0"][-1]
    assert 0 < mid < Nr - 1 and (c["R"][0] == c["R"][mid]).all() and (c["R"][Nr - 1] == c["R"][mid]).all()


@pytest.mark.parametrize("mutant", ref.RANK_MUTANTS)
def test_rank_mutants_are_rejected_by_the_lattice_comparison(lattice, mutant):
    assert any(not ref.ranks_equal(ref.rank(c["Q"], c["R"], c["t0"], c["t1"], mutant=mutant), c["want"]) for c in lattice), mutant


def test_partner_mutant_is_rejected(lattice):
    """j = i - s in place of j = i + s: other targets, other ranks"""
    c = lattice[3]
    n = c["R"].shape[0]
    assert c["Q"].shape[0] == n
    i = np.arange(n, dtype=np.int32)
    want = ref.rank(c["Q"], c["R"], i, ref.partner(n, 3))
    assert not ref.ranks_equal(ref.rank(c["Q"], c["R"], i, ref.partner(n, 3, mutant="minus")), want)
    assert ref.partner(5, 2).tolist() == [2, 3, 4, 0, 1]


@pytest.mark.parametrize("shape", ref.GAUSS_SHAPES)
def test_gaussian_bracket_decides_all_but_two_percent(shape):
    """the condition of the GPU test, on the float64 reference alone; the twin lies inside its own bracket; a mutant does not"""
    c = ref.gaussian_case(*shape)
    lo, hi = ref.rank_bracket(c["Q"], c["R"], c["t0"], c["t1"])
    want = ref.rank(c["Q"], c["R"], c["t0"], c["t1"])
    share = ref.undecided_share(lo, hi)
    print("gaussian %s: undecided share %.4f, ranks %d .. %d, rank 0 share %.3f" % (shape, share, want.min(), want.max(), float((want[:, 0] == 0).mean())))
    assert share <= ref.UNDECIDED_CAP
    assert ref.ranks_in_bracket(want, lo, hi, want)
    for mutant in ("swap_targets", "no_norm_r", "count_target"):
        assert not ref.ranks_in_bracket(ref.rank(c["Q"], c["R"], c["t0"], c["t1"], mutant=mutant), lo, hi, want), mutant


def test_level_twin_on_known_values():
    f32 = np.float32
    assert ref.level(f32(-1)) == 0 and ref.level(f32(1)) == 255 and ref.level(f32(np.nan)) == 0
    assert ref.level(f32(0.0)) == 128 and ref.level(f32(-0.0)) == 128     # 127.5: the tie goes to the even level
    assert ref.level(f32(2)) == 255 and ref.level(f32(-2)) == 0 and ref.level(f32(np.inf)) == 255 and ref.level(f32(-np.inf)) == 0
    lut = ref.make_lut()
    from split_vae_amd.data import ResidentDataset
    assert ref.bits_equal(lut, ResidentDataset.make_lut())
    for l in range(256):                                                   # the data's own values come back as their levels
        assert ref.level(lut[l]) == l
    # the fma is rounded once: against float64 arithmetic rounded twice the twin agrees except where that lands on a half level
    rng = np.random.default_rng(0)
    v = rng.uniform(-1, 1, 2000).astype(f32)
    naive = np.clip(np.rint(v.astype(np.float64) * 127.5 + 127.5), 0, 255).astype(np.int64)
    mine = np.array([ref.level(x) for x in v])
    assert (np.abs(mine - naive) <= 1).all() and (mine == naive).mean() > 0.99
    # the vectorised form takes the rational path only where float64 is not exact: the same levels, edge values included
    edge = ref.requantise_means(1, 8, 1)[..., :3].reshape(-1)
    assert np.isnan(edge).any() and (np.abs(edge) < 2.0 ** -20).any() and (np.abs(edge) > 1).any()
    for mutant in (None, "trunc"):
        assert ref.levels(edge, mutant).tolist() == [ref.level(x, mutant) for x in edge]
    assert ref.levels(v).tolist() == mine.tolist()


@pytest.mark.parametrize("mutant", ref.REQUANT_MUTANTS)
def test_requantise_mutants_are_rejected_by_the_bit_comparison(mutant):
    rejected = 0
    for n, (B, H, patch) in enumerate(ref.REQUANT_SHAPES[:6]):
        out6, perm = ref.requantise_means(B, H, 50 + n), ref.requantise_perms(B, H, patch, 60 + n)
        want = ref.requantise(out6, perm, patch)
        assert not np.isnan(want).any() and set(np.unique(want)) <= set(ref.make_lut().tolist())
        assert ref.bits_equal(want[..., :3].reshape(B, -1, 3)[0], want[..., 3:].reshape(B, -1, 3)[0])     # image 0: the identity
        rejected += not ref.bits_equal(ref.requantise(out6, perm, patch, mutant=mutant), want)
    assert rejected >= 1, mutant


def test_pair_mutant_is_rejected_by_the_bit_comparison():
    rng = np.random.default_rng(3)
    mu = rng.standard_normal((9, 7)).astype(np.float32)
    ig, il = np.array([0, 8, 3, 3], np.int32), np.array([5, 8, 1, 0], np.int32)
    want = ref.pair(mu, ig, il, 4)
    assert want.shape == (4, 7) and (want[2, :4] == mu[3, :4]).all() and (want[2, 4:] == mu[1, 4:]).all()
    assert not ref.bits_equal(ref.pair(mu, ig, il, 4, mutant="l_from_ig"), want)


def test_figure_arithmetic_against_the_twin():
    from split_vae_amd import swap
    rng = np.random.default_rng(5)
    ranks = rng.integers(0, 30, size=(3, 40, 2))
    ranks[1:, ::3, 0] = 0
    got, want = swap.figures(ranks, 10), ref.figures(ranks, 10)
    assert set(got) == set(want) == {"kept1", "keptk", "mrr", "leak1", "cycle1"}
    for key in want:
        assert abs(got[key] - want[key]) <= 1e-12, key
    assert swap.figures(np.zeros((2, 5, 2), np.int64), 1) == dict(kept1=1.0, keptk=1.0, mrr=1.0, leak1=1.0, cycle1=1.0)
    labels = rng.integers(0, 10, size=40)
    pred = rng.integers(0, 10, size=(3, 40))
    pred[1, ::2] = labels[::2]
    got, want = swap.class_figures(pred, labels, [3, 7]), ref.class_figures(pred, labels, [3, 7])
    assert got["unlike_pairs"] == want["unlike_pairs"] > 0
    for key in ("follows_g", "follows_l", "unswapped_acc"):
        assert abs(got[key] - want[key]) <= 1e-12, key
    same = swap.class_figures(np.zeros((2, 4), int), np.zeros(4, int), [1])
    assert same["unlike_pairs"] == 0 and same["follows_g"] is None and same["unswapped_acc"] == 1.0


def test_partner_shifts_come_from_the_host_philox_mirror(lib):
    from split_vae_amd import ops, swap
    for seed, p, a in ((0, 1, 0), (7, 3, 2), (2 ** 63 + 5, 8, 11)):
        assert ops.swap_shift_word_host(seed, p, a) == ref.shift_word(seed, p, a)
    for seed, n, P in ((0, 20, 2), (7, 9, 8), (123, 26032, 8), (5, 2, 1)):
        s = swap.partner_shifts(seed, n, P)
        assert s == ref.partner_shifts(seed, n, P) and len(set(s)) == P and min(s) >= 1 and max(s) <= n - 1
    assert swap.partner_shifts(1, 1000, 4) != swap.partner_shifts(2, 1000, 4)
    with pytest.raises(ValueError):
        swap.partner_shifts(0, 5, 5)
    with pytest.raises(ValueError):
        swap._check_shifts([3, 3], 20)
    with pytest.raises(ValueError):
        swap._check_shifts([20], 20)


# ---------------------------------------------------------------- the C ABI's argument checks (nothing is launched)
def test_entry_points_validate_arguments(lib):
    from split_vae_amd import _lib
    BAD, UNS, WS = _lib.STATUS_BADARG, _lib.STATUS_UNSUPPORTED, _lib.STATUS_WORKSPACE
    a = 1 << 20                                                            # a well aligned address nobody dereferences: every call below is refused
    n = C.c_int64(-1)
    assert lib.sv_swap_rank_workspace_bytes(64, 64, 32, None) == BAD
    assert lib.sv_swap_rank_workspace_bytes(0, 64, 32, C.byref(n)) == BAD and lib.sv_swap_rank_workspace_bytes(64, 64, 0, C.byref(n)) == BAD
    assert lib.sv_swap_rank_workspace_bytes(_lib.SWAP_MAX_NQ + 1, 64, 32, C.byref(n)) == UNS
    assert lib.sv_swap_rank_workspace_bytes(64, _lib.SWAP_MAX_NR + 1, 32, C.byref(n)) == UNS
    assert lib.sv_swap_rank_workspace_bytes(64, 64, _lib.SWAP_MAX_L + 1, C.byref(n)) == UNS and n.value == -1
    assert lib.sv_swap_rank_workspace_bytes(_lib.SWAP_MAX_NQ, 65536, 256, C.byref(n)) == 0 and n.value > 2 * _lib.SWAP_MAX_NQ * 256 * 4
    assert _lib.SWAP_MAX_L >= 256 and _lib.SWAP_MAX_NQ == 8 * 65536
    assert lib.sv_swap_rank_workspace_bytes(130, 5000, 33, C.byref(n)) == 0 and n.value % 256 == 0
    ok = [a, 33, a, 33, a, a, 130, 5000, 33, a, a, n.value, None]

    def rank(**kw):
        names = ("q", "ldq", "r", "ldr", "t0", "t1", "Nq", "Nr", "L", "rank", "ws", "bytes", "stream")
        args = list(ok)
        for key, v in kw.items():
            args[names.index(key)] = v
        return lib.sv_swap_rank(*args)

    for key in ("q", "r", "t0", "t1", "rank", "ws"):
        assert rank(**{key: None}) == BAD, key
        assert rank(**{key: a + 2}) == BAD, key
    assert rank(ws=a + 8) == BAD                                           # the workspace: 16 bytes
    assert rank(Nq=0) == BAD and rank(Nr=0) == BAD and rank(L=0) == BAD and rank(Nq=-1) == BAD
    assert rank(ldq=32) == BAD and rank(ldr=32) == BAD
    assert rank(L=513, ldq=600, ldr=600) == UNS and rank(Nq=_lib.SWAP_MAX_NQ + 1) == UNS
    assert rank(bytes=n.value - 1) == WS
    # sv_swap_pair
    assert lib.sv_swap_pair(None, 8, a, a, a, 0, 4, 2, 4, 4, None) == BAD and lib.sv_swap_pair(a, 8, None, a, a, 0, 4, 2, 4, 4, None) == BAD
    assert lib.sv_swap_pair(a, 8, a, a, None, 0, 4, 2, 4, 4, None) == BAD and lib.sv_swap_pair(a, 7, a, a, a, 0, 4, 2, 4, 4, None) == BAD
    assert lib.sv_swap_pair(a, 8, a, a, a, 7, 4, 2, 4, 4, None) == BAD and lib.sv_swap_pair(a, 8, a, a, a, 0, 0, 2, 4, 4, None) == BAD
    assert lib.sv_swap_pair(a, 8, a, a, a, 0, 4, 0, 4, 4, None) == BAD and lib.sv_swap_pair(a, 8, a, a, a, 0, 4, 2, 4, 0, None) == BAD
    assert lib.sv_swap_pair(a + 2, 8, a, a, a, 0, 4, 2, 4, 4, None) == BAD and lib.sv_swap_pair(a, 8, a, a, a + 2, 0, 4, 2, 4, 4, None) == BAD
    assert lib.sv_swap_pair(a, 8, a, a, a + 1, 1, 4, 2, 4, 4, None) == BAD
    # sv_swap_requantise: as sv_scramble_gather refuses
    b = a + (1 << 16)
    assert lib.sv_swap_requantise(None, a, a, b, 1, 8, 8, 4, None) == BAD and lib.sv_swap_requantise(a, None, a, b, 1, 8, 8, 4, None) == BAD
    assert lib.sv_swap_requantise(a, a, None, b, 1, 8, 8, 4, None) == BAD and lib.sv_swap_requantise(a, a, a, None, 1, 8, 8, 4, None) == BAD
    assert lib.sv_swap_requantise(a + 2, a, a, b, 1, 8, 8, 4, None) == BAD and lib.sv_swap_requantise(a, a, a, b + 2, 1, 8, 8, 4, None) == BAD
    assert lib.sv_swap_requantise(a, a, a, a, 1, 8, 8, 4, None) == BAD                       # in place
    assert lib.sv_swap_requantise(a, a, a, b, 0, 8, 8, 4, None) == BAD and lib.sv_swap_requantise(a, a, a, b, 1, 8, 8, 0, None) == BAD
    assert lib.sv_swap_requantise(a, a, a, b, 1, 8, 8, 3, None) == UNS and lib.sv_swap_requantise(a, a, a, b, 1, 8, 4, 2, None) == UNS


# ---------------------------------------------------------------- flags, parser, refusals, the line
WEIGHTS = ["--weights", "nowhere.npz"]


@pytest.mark.parametrize("flags,words", [
    (["--model", "gmvae"], "one latent block"),
    (["--augmentation", "blur"], "--augmentation blur"),
    (["--swap_partners", "0"], "--swap_partners P"),
    (["--swap_partners", "9"], "--swap_partners P"),
    (["--swap_images", "1"], "--swap_images N"),
    (["--swap_images", "3", "--swap_partners", "3"], "--swap_partners P"),
    (["--swap_k", "0"], "--swap_k K"),
    (["--swap_knn", "33"], "--swap_knn K"),
    (["--swap_knn", "5", "--swap_refs", "4"], "--swap_refs 4"),
    (["--swap_grid", "0"], "--swap_grid n"),
    (["--knn_probe", "5"], "runs the swap report only: --knn_probe"),
    (["--recon_quality", "8"], "runs the swap report only: --recon_quality"),
])
def test_refusals_print_their_message_before_any_device_work(monkeypatch, flags, words):
    import torch
    from split_vae_amd import data, swap

    def never(*a, **k):
        raise AssertionError("data or device work before the flags were checked")
    monkeypatch.setattr(data, "get_dataset", never)
    monkeypatch.setattr(torch.cuda, "is_available", never)
    with pytest.raises(SystemExit) as e:
        swap.main(WEIGHTS + flags)
    assert words in str(e.value)


def test_parser_has_the_flags_and_leaves_the_other_parsers_alone():
    from split_vae_amd import reports, swap
    from split_vae_amd.main import build_parser
    args = swap.build_parser().parse_args(WEIGHTS)
    assert (args.swap_images, args.swap_partners, args.swap_k, args.swap_knn, args.swap_refs, args.swap_out, args.swap_grid) == \
        (None, 1, 10, 5, 20000, None, 8)
    assert not hasattr(build_parser().parse_args([]), "swap_partners")
    assert not any(e.name.startswith("swap") for e in reports.TABLE)
    swap.check_flags("lgvae", "scramble", None, 1, 10, 5, 20000, 8, 128, 128)
    swap.check_flags("lggmvae", "no_op", 65536, 8, 1, 0, 0, 32, 512, 1)
    with pytest.raises(SystemExit):
        swap.check_flags("lgvae", "scramble", None, 1, 10, 5, 20000, 8, 513, 128)
    with pytest.raises(SystemExit):
        swap.check_flags("lgvae", "scramble", 65537, 1, 10, 5, 20000, 8)


def test_report_line_with_and_without_labels():
    from split_vae_amd import swap
    res = dict(n_images=26032, partners=2, k=10, labelled=False, follows_g=None)
    for s, base in (("g", 0.5), ("l", 0.25)):
        res.update({"kept1_" + s: base, "keptk_" + s: base + 0.125, "mrr_" + s: base + 0.0625, "leak1_" + s: base / 100, "cycle1_" + s: base + 0.25})
    bare = swap.report_line(res)
    assert bare == ("Test swap consistency (26032 images, 2 partners): z_g kept@1 0.5000, kept@10 0.6250, MRR 0.5625, leak@1 0.0050 (cycle@1 0.7500); "
                    "z_l kept@1 0.2500, kept@10 0.3750, MRR 0.3125, leak@1 0.0025 (cycle@1 0.5000)")
    res.update(labelled=True, follows_g=0.9, follows_l=0.05, unlike_pairs=46811, knn=5, n_ref=20000, unswapped_acc=0.93)
    assert swap.report_line(res) == bare + "; class follows z_g source 0.9000, z_l source 0.0500 (46811 unlike pairs, k=5, 20000 refs; unswapped 0.9300)"
    res["k"] = 3
    assert "kept@3 0.6250" in swap.report_line(res)
