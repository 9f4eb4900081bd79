"""CPU checks of training from cached visual tokens: the host refusals of the four new entry
points, the index / view validation of Model.forward_cached and TokenCache.fill, and the --cache_tokens options.  No
compute calls (no GPU here): every pointer below is refused before it is dereferenced."""
import pytest
import torch


def mini_model(**kw):
    import mmvqa_amd
    from oracle import mmbert_oracle as O
    d = dict(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=1, heads=12, vocab_size=50, emb_vocab=50,
             bert_max_pos=32, dataset="VQA-Med")
    d.update(kw)
    return mmvqa_amd.Model(O.make_args(**d))


def test_new_entry_points_refuse_bad_arguments_on_the_host():
    """each row is refused with MMVQA_ERR_ARG and its one sentence before any HIP call"""
    from mmvqa_amd import _lib as L
    lib = L.lib()
    p, q = 0x1000, 0x2000
    # gather: (stream, cache, N, K, idx, view, out, B, hidden, num_vis); scatter: (stream, vis, idx, view, cache, N, K, B, hidden, num_vis)
    table = (
        ("tokens_gather", (None, None, 4, 2, p, p, q, 3, 96, 5), b"tokens_gather: null pointer"),
        ("tokens_gather", (None, p, 4, 2, None, p, q, 3, 96, 5), b"tokens_gather: null pointer"),
        ("tokens_gather", (None, p, 4, 2, p, None, q, 3, 96, 5), b"tokens_gather: null pointer"),
        ("tokens_gather", (None, p, 4, 2, p, p, None, 3, 96, 5), b"tokens_gather: null pointer"),
        ("tokens_gather", (None, p, 4, 2, p, p, q, 3, 100, 5), b"tokens_gather: hidden=100 must be a multiple of 8, at most 1024"),
        ("tokens_gather", (None, p, 4, 2, p, p, q, 3, 1032, 5), b"tokens_gather: hidden=1032 must be a multiple of 8, at most 1024"),
        ("tokens_gather", (None, p, 4, 2, p, p, q, 3, 0, 5), b"tokens_gather: hidden=0 must be a multiple of 8, at most 1024"),
        ("tokens_gather", (None, p, 4, 2, p, p, q, 0, 96, 5), b"tokens_gather: B=0 N=4 K=2 num_vis=5 must all be at least 1"),
        ("tokens_gather", (None, p, 0, 2, p, p, q, 3, 96, 5), b"tokens_gather: B=3 N=0 K=2 num_vis=5 must all be at least 1"),
        ("tokens_gather", (None, p, 4, 0, p, p, q, 3, 96, 5), b"tokens_gather: B=3 N=4 K=0 num_vis=5 must all be at least 1"),
        ("tokens_gather", (None, p, 4, 2, p, p, q, 3, 96, 0), b"tokens_gather: B=3 N=4 K=2 num_vis=0 must all be at least 1"),
        ("tokens_gather", (None, p + 4, 4, 2, p, p, q, 3, 96, 5), b"tokens_gather: cache and token rows must be 16-byte aligned"),
        ("tokens_gather", (None, p, 4, 2, p, p, q + 8, 3, 96, 5), b"tokens_gather: cache and token rows must be 16-byte aligned"),
        ("tokens_scatter", (None, None, p, 0, q, 4, 2, 3, 96, 5), b"tokens_scatter: null pointer"),
        ("tokens_scatter", (None, p, None, 0, q, 4, 2, 3, 96, 5), b"tokens_scatter: null pointer"),
        ("tokens_scatter", (None, p, p, 0, None, 4, 2, 3, 96, 5), b"tokens_scatter: null pointer"),
        ("tokens_scatter", (None, p, p, 0, q, 4, 2, 3, 12, 5), b"tokens_scatter: hidden=12 must be a multiple of 8, at most 1024"),
        ("tokens_scatter", (None, p, p, 0, q, 4, 2, -1, 96, 5), b"tokens_scatter: B=-1 N=4 K=2 num_vis=5 must all be at least 1"),
        ("tokens_scatter", (None, p, p, 0, q + 4, 4, 2, 3, 96, 5), b"tokens_scatter: cache and token rows must be 16-byte aligned"),
        ("tokens_scatter", (None, p, p, 2, q, 4, 2, 3, 96, 5), b"tokens_scatter: view=2 is outside 0 .. K-1 = 1"),
        ("tokens_scatter", (None, p, p, -1, q, 4, 2, 3, 96, 5), b"tokens_scatter: view=-1 is outside 0 .. K-1 = 1"),
        ("engine_forward_cached", (None, None, p, 4, 2, p, p, p, p, p, p, 52, None, 1, 7), b"forward_cached: null pointer"),
        ("engine_backward_cached", (None, None, p, 52, None), b"backward_cached: null pointer"),
    )
    for name, args, what in table:
        rc = getattr(lib, "mmvqa_" + name)(*args)
        err = lib.mmvqa_last_error()
        assert rc == -1 and what in err, (name, what, rc, err)


def test_engine_cached_entry_points_refuse_by_state():
    """never planned: MMVQA_ERR_STATE (-3); a null pointer: MMVQA_ERR_ARG; the f16 operand mode: MMVQA_ERR_ARG whatever the
    engine's state; a backward without its forward: MMVQA_ERR_STATE"""
    from mmvqa_amd import _lib as L
    m = mini_model()
    lib, p = L.lib(), 0x1000
    fwd = lambda *a: lib.mmvqa_engine_forward_cached(m._handle, None, *a)   # noqa: E731
    assert fwd(p, 4, 2, p, p, p, p, p, p, 52, None, 1, 7) == -3
    assert b"engine_forward_cached: plan/bind first" in lib.mmvqa_last_error()
    for k in (0, 3, 4, 5, 6, 7, 8):                       # cache, idx, view, ids, seg, mask, logits
        a = [p, 4, 2, p, p, p, p, p, p, 52, None, 1, 7]
        a[k] = None
        assert fwd(*a) == -1 and b"forward_cached: null pointer" in lib.mmvqa_last_error(), k
    assert lib.mmvqa_engine_set_precision(m._handle, L.PREC_F16) == 0
    assert fwd(p, 4, 2, p, p, p, p, p, p, 52, None, 1, 7) == -1
    assert b"engine_forward_cached: runs with fp32 operands, not in the f16 operand mode" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_set_precision(m._handle, L.PREC_F32) == 0
    assert lib.mmvqa_engine_backward_cached(m._handle, None, p, 52, None) == -3
    assert b"engine_backward_cached: run mmvqa_engine_forward_cached first" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_backward_cached(m._handle, None, None, 52, None) == -1
    # planned (the plan needs no device), not bound: still a state error, for the forward and for its backward
    assert lib.mmvqa_engine_plan(m._handle, 3, 12, 64, 64) > 0
    assert fwd(p, 4, 2, p, p, p, p, p, p, 52, None, 1, 7) == -3
    assert lib.mmvqa_engine_backward_cached(m._handle, None, p, 52, None) == -3


def test_forward_cached_validates_index_and_view_on_the_host():
    """integers only, 0 <= index < N, 0 <= view < K, the batch's length, no device tensor: ValueError with the offending
    position, before the model asks where its inputs live (this model and its cache are on the CPU)"""
    from mmvqa_amd.model import cached_maps
    from mmvqa_amd.tokens import TokenCache
    m = mini_model()
    cache = TokenCache(m, 4, views=2)
    assert tuple(cache.tokens.shape) == (4, 2, 5, 96) and cache.nbytes == 4 * 2 * 5 * 96 * 4 and cache.fingerprint is None
    ids = torch.zeros(3, 12, dtype=torch.long)
    call = lambda index, view: m.forward_cached(cache, index, view, ids, ids, torch.ones_like(ids))   # noqa: E731
    for index, view, what in (
            ([0, 1, 4], [0, 0, 0], r"index\[2\] = 4 is outside the cache's 4 images"),
            ([0, -1, 2], [0, 0, 0], r"index\[1\] = -1 is outside"),
            ([0, 1, 2], [0, 2, 0], r"view\[1\] = 2 is outside the cache's 2 views"),
            ([0, 1, 2], [-1, 0, 0], r"view\[0\] = -1 is outside"),
            ([0, 1], [0, 0, 0], "index has 2 entries for 3 rows"),
            ([0, 1, 2], [0, 0, 0, 0], "view has 4 entries for 3 rows"),
            ([0, 1.5, 2], [0, 0, 0], "index must hold integers, not 1.5 at position 1"),
            ([0, 1, 2], [0, True, 0], "view must hold integers, not True at position 1"),
            (torch.tensor([0.0, 1.0, 2.0]), [0, 0, 0], "index must be a 1-d integer tensor"),
            ([0, 1, 2], torch.zeros(3, 1, dtype=torch.long), "view must be a 1-d integer tensor"),
            ([0, 1, 2], torch.zeros(3, dtype=torch.bool), "view must be a 1-d integer tensor")):
        with pytest.raises(ValueError, match=what):
            call(index, view)
    # valid maps: index then view, int32, one tensor; numpy integers and tensors are taken
    import numpy as np
    maps = cached_maps(torch.tensor([3, 0, 3]), [np.int64(1), 0, 1], 4, 2, 3)
    assert maps.dtype == torch.int32 and maps.tolist() == [3, 0, 3, 1, 0, 1]
    # ... and only then does the model refuse to compute on the CPU
    import mmvqa_amd
    with pytest.raises(mmvqa_amd.MMVQAError, match="GPU only"):
        call([3, 0, 3], [1, 0, 1])
    with pytest.raises(ValueError, match="the cache holds tokens"):
        mini_model(hidden_size=192).forward_cached(cache, [0, 1, 2], [0, 0, 0], ids, ids, ids)
    with pytest.raises(ValueError, match="at least one image and one view"):
        TokenCache(m, 4, views=0)
    # a fill names distinct rows of the cache and one of its views
    img = torch.zeros(2, 3, 32, 32)
    with pytest.raises(ValueError, match=r"index\[1\] = 1 repeats index\[0\]"):
        cache.fill([1, 1], img)
    with pytest.raises(ValueError, match=r"index\[0\] = 4 is outside"):
        cache.fill([4, 1], img)
    with pytest.raises(ValueError, match="index has 3 entries for 2 images"):
        cache.fill([0, 1, 2], img)
    with pytest.raises(ValueError, match="view = 2 is outside the cache's 2 views"):
        cache.fill([0, 1], img, view=2)
    with pytest.raises(mmvqa_amd.MMVQAError, match="has not been filled"):
        cache.check(m)


def test_token_range_and_freeze_visual():
    """transformer.trans.* is one contiguous range between the embeddings and the encoder; freeze_visual freezes exactly it"""
    m = mini_model()
    lo, hi = m.token_range()
    names = [n for n, _, l, h in m._param_ranges() if lo <= l and h <= hi]
    assert names and all(n.startswith("transformer.trans.") for n in names)
    assert sum(n.startswith("transformer.trans.") for n, _ in m.named_parameters()) == len(names)
    assert 0 < lo < hi < m.flat_params.numel()
    m.freeze_visual()
    assert all(p.requires_grad != n.startswith("transformer.trans.") for n, p in m.named_parameters())
    assert m._frozen_state()[0] == 3      # backbone without gradient, BatchNorms on running statistics


def test_cache_tokens_options():
    from mmvqa_amd.train import parse_args
    mode, a = parse_args(["vqa", "--cache_tokens"])
    assert mode == "vqa" and a.cache_tokens and a.cache_views is None and a.cache_images is None
    _, a = parse_args(["vqa", "--cache_tokens", "--cache_views", "3", "--cache_images", "40", "--clip", "--ema_decay", "0.9",
                       "--weight_decay", "0.01", "--smoothing", "0.1", "--watch", "parameters"])
    assert a.cache_views == 3 and a.cache_images == 40
    assert not parse_args(["vqa"])[1].cache_tokens


@pytest.mark.parametrize("argv,what", [
    (["vqa", "--cache_tokens", "--mixed_precision"], "--cache_tokens cannot be combined with --mixed_precision"),
    (["vqa", "--cache_tokens", "--group_by_image"], "--cache_tokens cannot be combined with --group_by_image"),
    (["mlm", "--cache_tokens"], "--cache_tokens is for vqa: caching visual tokens for mlm is not built"),
    (["supcon", "--cache_tokens"], "--cache_tokens is for vqa"),
    (["distill", "--cache_tokens"], "--cache_tokens is for vqa"),
    (["eval", "--cache_tokens"], "--cache_tokens is for vqa"),
    (["gradcam", "--cache_tokens"], "--cache_tokens is for vqa"),
    (["vqa", "--cache_views", "2"], "--cache_views is read with --cache_tokens only"),
    (["vqa", "--cache_images", "8"], "--cache_images is read with --cache_tokens only"),
    (["vqa", "--cache_tokens", "--cache_views", "0"], "--cache_views 0 must be at least 1"),
    (["vqa", "--cache_tokens", "--cache_images", "0"], "--cache_images 0 must be at least 1"),
])
def test_cache_tokens_refusals(argv, what, capsys):
    from mmvqa_amd.train import parse_args
    with pytest.raises(SystemExit):
        parse_args(argv)
    assert what in capsys.readouterr().err


def test_cache_tokens_refuses_more_than_one_process(monkeypatch, capsys):
    from mmvqa_amd.train import parse_args
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        parse_args(["vqa", "--cache_tokens"])
    assert "--cache_tokens runs in one process" in capsys.readouterr().err


# ----------------------------------------------------------------------------- --cache_tokens --data_dir: the host side
@pytest.fixture(scope="module")
def vqa_tree(tmp_path_factory):
    from test_hip_group_loop import make_grouped_vqa_tree
    return make_grouped_vqa_tree(str(tmp_path_factory.mktemp("vqa_cached")))


def test_cache_rows_follow_the_tables_images(vqa_tree):
    """image_of_rows numbers the distinct images in first-appearance order; VqaImageDataset item i is that image with
    index i (the cache row its tokens go to); every table row maps to the row of its own image"""
    from mmvqa_amd import data as D
    _cols, tabs, _ = D.vqa_tables(vqa_tree)
    for split, counts in (("train", (4, 3, 4)), ("val", (3, 1, 4))):
        rows = tabs[split]
        paths, image_of = D.image_of_rows(rows)
        assert len(paths) == len(counts) == len(set(paths)) and len(image_of) == len(rows) == sum(counts)
        assert [image_of.count(i) for i in range(len(counts))] == list(counts)
        assert all(rows[r][0] == paths[image_of[r]] for r in range(len(rows)))
        assert paths == [p for p, _ in D.group_rows_by_image(rows)]
        ds = D.VqaImageDataset(rows)
        assert len(ds) == len(counts) and ds.image_of == image_of
        for i in range(len(ds)):
            px, ids, _seg, _mask, _tgt, idx = ds[(0, i)]
            assert idx == i and px.dtype.name == "uint8" and px.shape[2] == 3 and tuple(ids.shape) == (1,)
            assert (px == D.decode(paths[i])).all()
        batch = D.collate([ds[(0, i)] for i in (2, 0)])
        assert batch["index"].tolist() == [2, 0] and batch["shapes"].shape == (2, 2)


def test_text_batches_decode_nothing(vqa_tree, monkeypatch):
    """VqaTextDataset: the text, answer and category of VqaDataset's item without its image; `image` names the cache row;
    no image is decoded, by the dataset or by a HostLoader over it"""
    from feeder_helpers import tokenizer
    from mmvqa_amd import data as D
    _cols, tabs, _ = D.vqa_tables(vqa_tree)
    rows, tok = tabs["train"], tokenizer()
    cats = D.category_ids(rows)
    full = D.VqaDataset(rows, tok, 16, categories=cats)
    items = [full[(0, r)] for r in range(len(rows))]                  # (decoded before decode is barred)

    def no_decode(path):
        raise AssertionError(f"{path} decoded after the fill")
    monkeypatch.setattr(D, "decode", no_decode)
    ds = D.VqaTextDataset(rows, tok, 16, categories=cats)
    _paths, image_of = D.image_of_rows(rows)
    for r, ref in enumerate(items):
        ids, seg, mask, ans, image, idx, cat = ds[(0, r)]
        assert torch.equal(ids, ref[1]) and torch.equal(seg, ref[2]) and torch.equal(mask, ref[3])
        assert int(ans) == int(ref[4]) and idx == r == ref[5] and cat == ref[6] and image == image_of[r]
    host = D.HostLoader(ds, 4, shuffle=True, seed=3, num_workers=0, pin_memory=False)
    host.set_epoch(1)
    seen = []
    for batch, params, meta in host:
        assert params is None and meta["epoch"] == 1 and "pixels" not in batch
        assert batch["ids"].shape[1] == 16 and batch["image"].dtype == torch.int64 and not batch["image"].is_cuda
        assert batch["image"].tolist() == [image_of[r] for r in batch["index"].tolist()]
        assert batch["category"].tolist() == [cats[rows[r][3]] for r in batch["index"].tolist()]
        seen += batch["index"].tolist()
    assert sorted(seen) == list(range(len(rows))) and seen != sorted(seen)
    plain = D.VqaTextDataset(rows, tok, 16)
    assert len(plain[(0, 0)]) == 6 and "category" not in D.collate_text([plain[(0, 0)], plain[(0, 1)]])
    with pytest.raises(ValueError, match="are not in the category map"):
        D.VqaTextDataset(rows, tok, 16, categories={})


def test_view_parameters_depend_on_seed_image_and_view_only(vqa_tree):
    """ViewLoader: file order; view 0 carries no augment parameters, view v >= 1 carries view_params(seed, image, v) --
    the same whatever the batch size"""
    from mmvqa_amd import data as D
    _cols, tabs, _ = D.vqa_tables(vqa_tree)
    images = D.VqaImageDataset(tabs["train"])

    def params(batch_size, view, seed=5):
        out = {}
        for batch, prm, meta in D.ViewLoader(images, batch_size, view, seed=seed, num_workers=0, aug=D.VQA_AUG, size=32):
            assert meta["epoch"] == view
            for k, i in enumerate(batch["index"].tolist()):
                out[i] = None if prm is None else prm[k]
        assert list(out) == [0, 1, 2]                                  # file order
        return out
    assert all(v is None for v in params(2, 0).values())
    a, b = params(2, 1), params(3, 1)
    assert a == b and all(a[i] == D.view_params(5, i, 1, 32, D.VQA_AUG) for i in a)
    assert a[0] != a[1] and a != params(2, 2) and a != params(2, 1, seed=6)


def test_cache_tokens_with_data_dir_parses():
    from mmvqa_amd.train import parse_args
    _, a = parse_args(["vqa", "--cache_tokens", "--cache_views", "2", "--data_dir", "VQA-Med", "--vocab_file", "vocab.txt"])
    assert a.cache_tokens and a.data_dir == "VQA-Med"


def test_cache_images_is_for_synthetic_runs(capsys):
    from mmvqa_amd.train import parse_args
    with pytest.raises(SystemExit):
        parse_args(["vqa", "--cache_tokens", "--cache_images", "8", "--data_dir", "VQA-Med"])
    assert "--cache_images sizes the synthetic train set" in capsys.readouterr().err
