"""data.pack_batches: first-fit packing of unpadded samples into (micro_bsz, ctx_len) rows of whole 16-token chunks."""
import pytest
import torch

from visualrwkv_amd.data import IGNORE_INDEX, build_sample, pack_batches


def _sample(i, n, n_img=0):
    d = dict(input_ids=torch.arange(1, n + 1) + 1000 * i, labels=torch.arange(1, n + 1) + 1000 * i, sample_id=f"s{i}", input_text=str(i))
    if n_img:
        d["images"] = {"dino": torch.full((n_img, 3, 2, 2), float(i)), "siglip": torch.full((n_img, 3, 2, 2), float(i))}
    return d


STREAM = [(40, 1), (100, 0), (17, 2), (200, 1), (5, 0), (96, 0), (16, 1)]


def _stream():
    return [_sample(i, n, k) for i, (n, k) in enumerate(STREAM)]


def test_every_token_once_in_order_and_layout_invariants():
    ctx, mb = 96, 2
    batches = list(pack_batches(_stream(), mb, ctx))
    seen = []
    for b in batches:
        assert b["input_ids"].shape == b["labels"].shape == (mb, ctx)
        assert sum(len(r) for r in b["sample_id"]) == b["n_samples"]
        for r in range(mb):
            lens = b["seg_lens"][r]
            assert sum(lens) == ctx and all(n > 0 and n % 16 == 0 for n in lens)
            assert len(lens) in (len(b["sample_id"][r]), len(b["sample_id"][r]) + 1)       # + a pad-only tail
            t = 0
            for j, n in enumerate(lens):
                assert int(b["labels"][r, t]) == IGNORE_INDEX                             # first token of every segment
                if j < len(b["sample_id"][r]):
                    i = int(b["sample_id"][r][j][1:])
                    m = min(STREAM[i][0], ctx)                                             # a sample longer than ctx_len is cut
                    want = torch.arange(1, m + 1) + 1000 * i
                    assert torch.equal(b["input_ids"][r, t:t + m], want)
                    assert torch.equal(b["labels"][r, t + 1:t + m], want[1:])
                    assert n == -(-m // 16) * 16
                    assert (b["input_ids"][r, t + m:t + n] == 0).all() and (b["labels"][r, t + m:t + n] == IGNORE_INDEX).all()
                    seen.append(i)
                else:                                                                      # pad-only tail segment
                    assert (b["input_ids"][r, t:] == 0).all() and (b["labels"][r, t:] == IGNORE_INDEX).all()
                t += n
    assert sorted(seen) == list(range(len(STREAM)))
    # first fit in arrival order; the batch closes at the first sample that fits no row; the stream ends mid-batch
    assert [b["sample_id"] for b in batches] == [[["s0", "s2"], ["s1"]], [["s3"], ["s4"]], [["s5"], ["s6"]]]
    assert batches[0]["seg_lens"] == [[48, 32, 16], [96]] and batches[1]["seg_lens"] == [[96], [16, 80]]
    assert batches[2]["seg_lens"] == [[96], [16, 80]]


def test_images_come_in_row_then_position_order():
    b = list(pack_batches(_stream(), 2, 96))
    assert b[0]["images"]["num_image_per_sample"] == [1, 2]
    assert b[0]["images"]["dino"][:, 0, 0, 0].tolist() == [0.0, 2.0, 2.0] and b[0]["images"]["siglip"].shape[0] == 3
    # arrival order 0, 1, 2 but sample 1 sits in row 1: its images come after those of row 0
    s = [_sample(0, 80, 1), _sample(1, 80, 1), _sample(2, 16, 1)]
    one = next(pack_batches(s, 2, 96))
    assert one["sample_id"] == [["s0", "s2"], ["s1"]] and one["images"]["dino"][:, 0, 0, 0].tolist() == [0.0, 2.0, 1.0]
    assert "images" not in list(pack_batches([_sample(0, 20)], 1, 32))[0]


def test_deterministic_and_validates():
    a, b = list(pack_batches(_stream(), 2, 96)), list(pack_batches(_stream(), 2, 96))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x["input_ids"], y["input_ids"]) and torch.equal(x["labels"], y["labels"]) and x["seg_lens"] == y["seg_lens"]
    with pytest.raises(ValueError):
        next(pack_batches(_stream(), 2, 100))
    assert list(pack_batches([], 2, 96)) == []


def test_layout_of_a_packed_batch():
    from visualrwkv_amd.visual import VisualRWKV
    b = next(pack_batches(_stream(), 2, 96))
    lay = VisualRWKV.packed_layout(b, "cpu")
    assert lay.n_samples == 3 and lay.n_segments == 4
    assert lay.first.view(2, 96).nonzero().tolist() == [[0, 0], [0, 48], [0, 80], [1, 0]]
    assert VisualRWKV.packed_layout({"input_ids": b["input_ids"]}, "cpu") is None


def test_build_sample_passes_the_padding_switch_through():
    class Tok:
        def encode(self, s):
            return [ord(c) % 250 + 1 for c in s]
    rec = {"id": "r0", "conversations": [{"from": "human", "value": "hi there"}, {"from": "gpt", "value": "hello"}]}
    padded = build_sample(rec, Tok(), 64, 16)
    raw = build_sample(rec, Tok(), 64, 16, do_pad_to_max_length=False)
    n = len(raw["input_ids"])
    assert len(padded["input_ids"]) == 64 and 0 < n < 64
    assert torch.equal(padded["input_ids"][:n], raw["input_ids"]) and torch.equal(padded["labels"][:n], raw["labels"])
