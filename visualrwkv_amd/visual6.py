"""VisualRWKV-6 (BASELINE config 4) around the RWKV-6 stack: mirror of VisualRWKV-v6/v6.0/src/model.py:339-560.

CLIP ViT-L/14 features (any module returning `.last_hidden_state` with a leading CLS token), `grid_pooling`, a linear
projector, the image span inserted after the left-padded first text part (`preparing_embedding`), and the
"bidirectional" pass that flips the image span on odd layers (`bidirectional_forward`).  Loss = the v7 one
(`training_step`, model.py:441-458 is the same code).

`args.image_state = 1` selects the v6.xx model instead (VisualRWKV-v6/v6.xx/src/model.py:321-343,429-495, "state tuning"): the image is
not part of the context.  Every Block first runs over the projected image features from a zero WKV state, and the state that pass ends
in is the initial state of the same Block's pass over the text (`preparing_embedding_state`, `unidirectional_forward`, `generate`).
The projector is trained only through dL/dS (wkv6.RUN_CUDA_RWKV6_STATE).  The default 0 is the bidirectional model above."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .rwkv6 import RWKV
from .rwkv7 import IGNORE_INDEX, L2Wrap

IMAGE_TOKEN_INDEX = -200       # VisualRWKV-v6/v6.0/src/dataset.py (v7 moved it to 65535)


class VisualRWKV6(nn.Module):
    def __init__(self, args, vit: nn.Module, vit_hidden_size: int):
        """`vit`: the frozen vision tower (the reference builds `CLIPVisionModel.from_pretrained(args.vision_tower_name)`,
        model.py:346; pass that model, or any module with the same output attribute)."""
        super().__init__()
        self.args = args
        self.rwkv = RWKV(args)
        self.vit = vit
        self.vit.requires_grad_(False)
        self.proj = nn.Linear(vit_hidden_size, args.n_embd, bias=False)
        self.img_start = self.img_end = 0

    def freeze_rwkv(self, num_layers_to_freeze):
        if num_layers_to_freeze == self.args.n_layer:
            self.rwkv.requires_grad_(False)
        for i, block in enumerate(self.rwkv.blocks):
            block.requires_grad_(i >= num_layers_to_freeze)

    def freeze_emb(self):
        self.rwkv.emb.requires_grad_(False)

    def freeze_proj(self):
        self.proj.requires_grad_(False)

    # ---- model.py:401-427
    def forward(self, samples, wkv=None):
        if getattr(self.args, "image_state", 0):
            x, targets, image_features = self.preparing_embedding_state(samples)
            return self.unidirectional_forward(x, image_features, wkv), targets
        x, targets, _ = self.preparing_embedding(samples)
        return self.bidirectional_forward(x, wkv), targets

    # ---- v6.xx model.py:326-343
    def unidirectional_forward(self, x, x_emb, wkv=None):
        """x: the text embeddings (B,T,C); x_emb: the projected image features (B,L,C).  `wkv`: a callable with RUN_CUDA_RWKV6_STATE's
        signature (tests pass the oracle)."""
        args = self.args
        if args.dropout > 0:
            x = self.rwkv.drop0(x)
        h = self.rwkv.forward_state(x, x_emb, wkv)
        if getattr(args, "fused", False) and h.is_cuda and self.rwkv.head.weight.dtype == torch.bfloat16:
            from . import fused
            return fused.linear(self.rwkv.head, h)
        return self.rwkv.head(h)

    def image_states(self, x_emb, wkv=None):
        """The per-layer WKV states the image pass ends in: [(B,H,64,64) f32] * n_layer."""
        states = []
        for block in self.rwkv.blocks:
            x_emb, state = block.forward_state(x_emb, None, wkv)
            states.append(state)
        return states

    def text_forward(self, x, states, wkv=None):
        """The text pass alone, from the states of `image_states`: the logits `unidirectional_forward` gives."""
        for block, state in zip(self.rwkv.blocks, states):
            x, _ = block.forward_state(x, state, wkv, False)
        return self.rwkv.head(self.rwkv.ln_out(x))

    @torch.no_grad()
    def generate(self, input_ids, images, do_sample, temperature, top_p, max_new_tokens, stop_token_idx, wkv=None):
        """Greedy generation of one sample in image-state mode (v6.xx model.py:468-495, which calls a method that file does not have: this
        is its intent).  The per-layer image states are computed once; the text pass is re-run from them for every new token
        (`generate_stateful` carries the state instead: one row per new token, and both models)."""
        if not getattr(self.args, "image_state", 0):
            raise NotImplementedError("generate is built for args.image_state = 1")
        if do_sample:
            raise NotImplementedError
        samples = {"input_ids": input_ids, "images": images, "labels": torch.full_like(input_ids, IGNORE_INDEX)}
        x, _, image_features = self.preparing_embedding_state(samples, truncate=False)
        states = self.image_states(image_features, wkv)
        generated = []
        for _ in range(max_new_tokens):
            next_token = torch.argmax(self.text_forward(x, states, wkv)[:, -1, :], dim=-1, keepdim=True)
            generated.append(next_token.item())
            if generated[-1] == stop_token_idx:
                break
            x = torch.cat((x, self.rwkv.emb(next_token)), dim=-2)[:, -self.args.ctx_len:, :]
        return generated

    @torch.no_grad()
    def prefill_state(self, input_ids, images, wkv=None):
        """The prompt's pass for stateful generation: -> (logits of the last row (1,V), an RWKV6State behind the whole prompt).
        image_state = 1: the image pass gives every layer's S, the shift rows start at zero (v6.xx has no shift across the image / text
        boundary), one pass over the text from there.  image_state = 0: `bidirectional_forward` over the prompt, keeping what every layer
        ends in -- on odd layers that is the state behind the flipped image span and the text after it; what follows the span is causal
        in every layer, so the steps after this are the plain ones."""
        from .rwkv6 import RWKV6State
        samples = {"input_ids": input_ids, "images": images, "labels": torch.full_like(input_ids, IGNORE_INDEX)}
        if getattr(self.args, "image_state", 0):
            x, _, image_features = self.preparing_embedding_state(samples, truncate=False)
            state = RWKV6State(self.args, x.size(0), x.device, x.dtype)
            for S, s_img in zip(state.S, self.image_states(image_features, wkv)):
                S.copy_(s_img)
            logits, state = self.rwkv.forward_stateful(x, state, last_only=True, wkv=wkv)
            return logits, state
        x, _, _ = self.preparing_embedding(samples, truncate=False)
        state = RWKV6State(self.args, x.size(0), x.device, x.dtype)
        s, e = self.img_start, self.img_end
        for i, block in enumerate(self.rwkv.blocks):
            rev = i % 2 == 1
            if rev:
                x = torch.cat((x[:, :s], x[:, s:e].flip(1), x[:, e:]), dim=1)
            x = block.forward_stateful(x, state, wkv)
            if rev:
                x = torch.cat((x[:, :s], x[:, s:e].flip(1), x[:, e:]), dim=1)
        state.n_tokens = x.size(1)
        return self.rwkv.head(self.rwkv.ln_out(x[:, -1])), state

    @torch.no_grad()
    def generate_stateful(self, input_ids, images, do_sample, temperature, top_p, max_new_tokens, stop_token_idx, use_graph=None, wkv=None):
        """`generate` with a carried state, for both models: one pass over the prompt (`prefill_state`), then one token per step -- a new
        token costs one row, not a pass over everything before it.  Returns what `generate` returns (the context is not cut to ctx_len:
        the state has no window).  use_graph: replay the step from a captured HIP graph (`RWKV.decoder_for`); None = where the decode
        step runs (bf16 on the GPU with args.fused)."""
        if do_sample:
            raise NotImplementedError
        logits, state = self.prefill_state(input_ids, images, wkv)
        if use_graph is None:
            use_graph = bool(getattr(self.args, "fused", False)) and wkv is None and logits.is_cuda and logits.dtype == torch.bfloat16
        step = self.rwkv.decoder_for(state) if use_graph else \
            (lambda x_emb: self.rwkv.forward_stateful(x_emb, state, last_only=True, wkv=wkv)[0])
        generated = []
        for i in range(max_new_tokens):
            next_token = torch.argmax(logits, dim=-1, keepdim=True)
            generated.append(next_token.item())
            if generated[-1] == stop_token_idx or i == max_new_tokens - 1:
                break
            logits = step(self.rwkv.emb(next_token))
        return generated

    def bidirectional_forward(self, x, wkv=None):
        args = self.args
        if args.dropout > 0:
            x = self.rwkv.drop0(x)
        s, e = self.img_start, self.img_end
        for i, block in enumerate(self.rwkv.blocks):
            rev = i % 2 == 1
            if rev:                                                    # odd layers read the image span right to left
                x = torch.cat((x[:, :s], x[:, s:e].flip(1), x[:, e:]), dim=1)
            if args.grad_cp >= 1 and torch.is_grad_enabled():      # 2 (the v7 fused path's selective mode) means 1 here
                from torch.utils.checkpoint import checkpoint
                x = checkpoint(block, x, wkv, use_reentrant=False)
            else:
                x = block(x, wkv)
            if rev:
                x = torch.cat((x[:, :s], x[:, s:e].flip(1), x[:, e:]), dim=1)
        if getattr(args, "fused", False) and x.is_cuda and self.rwkv.head.weight.dtype == torch.bfloat16:
            from . import fused
            return fused.linear(self.rwkv.head, self.rwkv.ln_out(x))           # input gradient in the forward GEMMs' layout
        return self.rwkv.head(self.rwkv.ln_out(x))

    def training_step(self, batch, batch_idx=0, wkv=None):
        logits, targets = self(batch, wkv)
        if getattr(self.args, "fused", False):
            from . import fused
            if fused.ce_supported(logits):                                      # one-pass shifted CE + L2Wrap (csrc/loss_fused.hip)
                return fused.loss_from_logits(logits, targets, IGNORE_INDEX)
        shift_logits = logits[..., :-1, :].contiguous()
        shift_labels = targets[..., 1:].contiguous()
        valid = torch.max((shift_labels != IGNORE_INDEX).sum(1), torch.ones_like(shift_labels[:, 0]))
        loss = F.cross_entropy(shift_logits.view(-1, shift_logits.size(-1)), shift_labels.view(-1),
                               ignore_index=IGNORE_INDEX, reduction="none")
        loss = (loss.view(shift_labels.size()).sum(1) / valid).mean()
        return L2Wrap.apply(loss, logits)

    # ---- model.py:466-485
    def encode_images(self, images):
        B, n_img, C, H, W = images.shape
        feats = self.vit(images.view(B * n_img, C, H, W)).last_hidden_state
        feats = feats.view(B, n_img, feats.shape[1], feats.shape[2])[:, 0]
        return self.proj(self.grid_pooling(feats))

    def grid_pooling(self, image_features):
        cls_features = image_features[:, 0:1, :]
        image_features = image_features[:, 1:, :]
        gs = self.args.grid_size
        if gs == -1:
            return torch.cat((image_features, cls_features), dim=1)
        if gs == 0:
            return cls_features
        if gs == 1:
            return torch.cat((image_features.mean(dim=1, keepdim=True), cls_features), dim=1)
        B, L, D = image_features.shape
        side = int(L ** 0.5)
        stride = side // gs
        pooled = F.avg_pool2d(image_features.view(B, side, side, D).permute(0, 3, 1, 2), kernel_size=stride, stride=stride)
        return torch.cat((pooled.permute(0, 2, 3, 1).reshape(B, -1, D), cls_features), dim=1)

    # ---- model.py:487-560: [left-padded first text part | image features (+CLS) | rest of the text]
    def preparing_embedding(self, samples, truncate=True):
        ids, labels = samples["input_ids"], samples["labels"]
        device = labels.device
        image_features = self.encode_images(samples["images"])
        is_img = ids == IMAGE_TOKEN_INDEX
        n_img = is_img.sum(1)
        if int(n_img.max()) > 1:
            raise ValueError("Too many images in one sample, should be 0 or 1.")
        pos = torch.where(n_img == 1, is_img.int().argmax(1), torch.zeros_like(n_img))
        max_pos = int(pos.max())
        self.img_start = max_pos
        self.img_end = max_pos + (image_features.shape[1] - 1)                 # CLS excluded
        embeds, new_labels = [], []
        for b in range(ids.shape[0]):
            p = int(pos[b])
            head_ids = torch.zeros(max_pos, dtype=ids.dtype, device=device)
            head_lab = torch.full((max_pos,), IGNORE_INDEX, dtype=labels.dtype, device=device)
            feats = image_features[b]
            if int(n_img[b]) == 1:
                if p > 0:
                    head_ids[-p:] = ids[b, :p]
                    head_lab[-p:] = labels[b, :p]
                tail_ids, tail_lab = ids[b, p + 1:], labels[b, p + 1:]
            else:
                feats = torch.zeros_like(feats)
                tail_ids, tail_lab = ids[b], labels[b]
            embeds.append(torch.cat((self.rwkv.emb(head_ids), feats, self.rwkv.emb(tail_ids))))
            new_labels.append(torch.cat((head_lab, torch.full((feats.shape[0],), IGNORE_INDEX, dtype=labels.dtype, device=device),
                                         tail_lab)))
        if truncate:                                   # keep the beginning unless it carries no label (model.py:496-509)
            L = self.args.ctx_len
            for i, (x, y) in enumerate(zip(embeds, new_labels)):
                if bool((y[:L] != IGNORE_INDEX).any()):
                    embeds[i], new_labels[i] = x[:L], y[:L]
                else:
                    embeds[i], new_labels[i] = x[-L:], y[-L:]
        max_len = max(x.shape[0] for x in embeds)
        out = torch.zeros(len(embeds), max_len, self.args.n_embd, dtype=samples["images"].dtype, device=device)
        lab = torch.full((len(embeds), max_len), IGNORE_INDEX, dtype=labels.dtype, device=device)
        for i, (x, y) in enumerate(zip(embeds, new_labels)):
            out[i, :x.shape[0]] = x
            lab[i, :y.shape[0]] = y
        return out, lab, image_features

    # ---- v6.xx model.py:414-466: the text is what stands right of the image token; the image is returned beside it
    def preparing_embedding_state(self, samples, truncate=True):
        ids, labels = samples["input_ids"], samples["labels"]
        device = labels.device
        image_features = self.encode_images(samples["images"])
        n_img = (ids == IMAGE_TOKEN_INDEX).sum(1)
        if int(n_img.max()) > 1:
            raise ValueError("Too many images in one sample, should be 0 or 1.")
        # a sample without an image gets zeroed features
        image_features = torch.where((n_img == 1).view(-1, 1, 1), image_features, torch.zeros_like(image_features))
        embeds, new_labels = [], []
        for b in range(ids.shape[0]):
            start = int((ids[b] == IMAGE_TOKEN_INDEX).int().argmax()) + 1 if int(n_img[b]) == 1 else 0
            embeds.append(self.rwkv.emb(ids[b, start:]))
            new_labels.append(labels[b, start:])
        if truncate:                                   # truncate_input: keep the beginning unless it carries no label
            L = self.args.ctx_len
            for i, (x, y) in enumerate(zip(embeds, new_labels)):
                if bool((y[:L] != IGNORE_INDEX).any()):
                    embeds[i], new_labels[i] = x[:L], y[:L]
                else:
                    embeds[i], new_labels[i] = x[-L:], y[-L:]
        max_len = max(x.shape[0] for x in embeds)
        out = torch.zeros(len(embeds), max_len, self.args.n_embd, dtype=samples["images"].dtype, device=device)
        lab = torch.full((len(embeds), max_len), IGNORE_INDEX, dtype=labels.dtype, device=device)
        for i, (x, y) in enumerate(zip(embeds, new_labels)):
            out[i, :x.shape[0]] = x
            lab[i, :y.shape[0]] = y
        return out, lab, image_features
