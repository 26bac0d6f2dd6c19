"""VisualRWKV-7: ViT features -> pool -> projector -> scatter into the token embeddings -> RWKV-7 LM.

Mirror of VisualRWKV-v7/v7.00/src/model.py:328-530 (`MLPWithContextGating`, `VisualRWKV`) without the
Lightning/DeepSpeed base classes: same constructor argument object, same sub-module names
(`rwkv`, `vit`, `proj`, `pool` => same state-dict keys), same batch-dict schema
(`input_ids`, `labels`, `images{dino,siglip,sam,...}`, `sample_id`; src/dataset.py:24-36), same loss.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn
from torch.nn import functional as F

from .rwkv7 import IGNORE_INDEX, IMAGE_TOKEN_INDEX, L2Wrap, L2WrapWindow, RWKV, TrainCarry, VRWKV, VisualTokenCompressor
from .vit import SamDinoSigLIPViTBackbone


class MLPWithContextGating(nn.Module):
    """LayerNorm(o_proj(x * sigmoid(gate(x))))   (src/model.py:328-338)"""

    def __init__(self, in_dim, n_embd):
        super().__init__()
        self.gate = nn.Linear(in_dim, in_dim, bias=False)
        self.o_proj = nn.Linear(in_dim, n_embd, bias=False)
        self.ln_v = nn.LayerNorm(n_embd)

    def forward(self, x):
        return self.ln_v(self.pre_norm(x))

    def pre_norm(self, x):
        """o_proj(x * sigmoid(gate(x))): everything before ln_v.  On the GPU the gate is one streaming HIP kernel and
        ln_v is fused with the scatter into the token embeddings by the caller (VisualRWKV.preparing_embedding)."""
        from . import fused
        if fused.visual_supported(x) and self.gate.weight.dtype == torch.bfloat16:
            return self.o_proj(fused.gate(x, self.gate(x)))
        return self.o_proj(x * torch.sigmoid(self.gate(x)))


def _embed(model, samples):
    """(input embeddings, labels, keyword arguments of model.rwkv(...) for the image mask: none without args.modality_ffn, the ImageNet logits of
    the RWKV vision encoder or None).  A batch may carry `n_image_tokens`, the count of IMAGE_TOKEN_INDEX in input_ids taken on the host (the
    collate): the routed path then needs no device synchronisation to size its two GEMMs."""
    res = model.preparing_embedding(samples)
    if len(res) == 2:
        return res[0], res[1], {}, None
    mk = {} if res[2] is None else {"mask": res[2], "n_image": samples.get("n_image_tokens")}
    return res[0], res[1], mk, (res[3] if len(res) > 3 else None)


class VisualRWKV(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.rwkv = RWKV(args)
        if len(getattr(args, "load_model", "")) > 0:
            self.from_pretrained(args.load_model)
        if int(getattr(args, "n_vrwkv_layer", 0) or 0) > 0:
            # v7.10 (src/model.py:419-424): encoder-free -- the trainable RWKV vision encoder takes the place of the frozen towers, the projector and
            # the pool; with args.modality_ffn = 1 this is the reference's model
            if int(getattr(args, "n_vtc_layer", 0) or 0) > 0:
                raise NotImplementedError("args.n_vrwkv_layer together with args.n_vtc_layer: the compressor follows the projector of the frozen "
                                          "towers (v7.03 / v7.04), which the RWKV vision encoder (v7.10) replaces")
            self.vrwkv = VRWKV(args)
            return
        self.vit = SamDinoSigLIPViTBackbone(getattr(args, "vision_tower_path", None),
                                            towers=getattr(args, "vision_towers", ("dino", "siglip", "sam")),
                                            default_image_size=getattr(args, "vision_image_size", 448),
                                            tower_kwargs=getattr(args, "vision_tower_kwargs", None))
        self.freeze_vit()
        if getattr(args, "proj_type", "mlp") == "linear":
            self.proj = nn.Linear(self.vit.embed_dim, args.n_embd, bias=False)
        else:
            self.proj = MLPWithContextGating(self.vit.embed_dim, args.n_embd)
        self.pool = nn.AdaptiveAvgPool2d(int(args.num_token_per_image ** 0.5))
        if int(getattr(args, "n_vtc_layer", 0) or 0) > 0:
            # v7.03 / v7.04 (src/model.py:401-403): the trainable compressor after the projector takes the place of the fixed 2-D pool before it
            if getattr(args, "modality_ffn", 0):
                raise NotImplementedError("args.n_vtc_layer together with args.modality_ffn: the compressor belongs to v7.03 / v7.04, the image "
                                          "experts to v7.10; no reference model has both")
            if getattr(args, "proj_type", "mlp") == "linear":
                raise NotImplementedError("args.n_vtc_layer with proj_type = 'linear': the compressor follows MLPWithContextGating's ln_v")
            self.vtc = VisualTokenCompressor(args)

    @property
    def has_vtc(self):
        return getattr(self, "vtc", None) is not None

    @property
    def has_vrwkv(self):
        return getattr(self, "vrwkv", None) is not None

    def init_vtc_weights(self):
        """Start the compressor from the language model (src/model.py:406-412): ln_out and the first n_vtc_layer Blocks, copied.  Call it after the
        language model's weights are loaded."""
        if not self.has_vtc:
            raise ValueError("init_vtc_weights: the model has no compressor (build it with args.n_vtc_layer > 0)")
        self.vtc.ln_out.load_state_dict(self.rwkv.ln_out.state_dict())
        for i in range(self.args.n_vtc_layer):
            self.vtc.blocks[i].load_state_dict(self.rwkv.blocks[i].state_dict())

    def from_pretrained(self, path):
        """Load the language model's weights.  With args.modality_ffn the checkpoint may be a v7.00 one without `ffn_v` / `ln_v`: non-strict, as
        v7.10 loads it (src/model.py:426-427); those keep their initialisation.  Anything else missing or unexpected is still an error."""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if not getattr(self.args, "modality_ffn", 0):
            self.rwkv.load_state_dict(sd)
            return
        res = self.rwkv.load_state_dict(sd, strict=False)
        bad = [k for k in res.missing_keys if ".ffn_v." not in k and ".ln_v." not in k] + list(res.unexpected_keys)
        if bad:
            raise RuntimeError(f"from_pretrained: keys that do not match the model: {bad[:8]}{' ...' if len(bad) > 8 else ''}")

    # ---- freezing helpers (src/model.py:368-388)
    def enable_pretrain_mode(self):
        """v7.10's pre-training stage (src/model.py:438-443): the RWKV vision encoder trainable, the language model frozen except the image
        experts `ffn_v` / `ln_v` of every Block, if it has them."""
        if not getattr(self.args, "modality_ffn", 0) and not self.has_vrwkv:
            raise ValueError("enable_pretrain_mode: the model has no ffn_v / ln_v (build it with args.modality_ffn = 1) and no vision encoder "
                             "(args.n_vrwkv_layer > 0)")
        if self.has_vrwkv:
            self.vrwkv.requires_grad_(True)
        self.rwkv.requires_grad_(False)
        for n, p in self.rwkv.named_parameters():
            if "ffn_v" in n or "ln_v" in n:
                p.requires_grad_(True)

    def freeze_vit(self):
        if self.has_vrwkv:
            raise ValueError("freeze_vit: the model has no frozen towers (args.n_vrwkv_layer > 0); freeze `vrwkv` itself if that is meant")
        self.vit.requires_grad_(False)

    def freeze_rwkv(self, num_layers_to_freeze):
        if num_layers_to_freeze == self.args.n_layer:
            self.rwkv.requires_grad_(False)
        for i, block in enumerate(self.rwkv.blocks):
            block.requires_grad_(i >= num_layers_to_freeze)

    def freeze_emb(self):
        self.rwkv.emb.requires_grad_(False)

    def freeze_proj(self):
        self.proj.requires_grad_(False)

    def freeze_for_state_tuning(self):
        """State tuning (args.state_tune; not in the reference): every weight frozen, only the learnable initial WKV states
        (`time_state` of every RWKV_Tmix_x070) train."""
        states = [n for n, _ in self.named_parameters() if n.endswith(".time_state")]
        if not states:
            raise ValueError("freeze_for_state_tuning: the model has no time_state parameters (build it with args.state_tune = 1)")
        for n, p in self.named_parameters():
            p.requires_grad_(n.endswith(".time_state"))

    def optimizer_groups(self):
        """Parameter groups of configure_optimizers (src/model.py:390-410): tensors that are at least 2-D
        after squeeze() get weight decay, everything else none.  The learnable initial states (`time_state`, args.state_tune) are a
        starting point of the recurrence, not a weight: no decay."""
        named = [(n, p) for n, p in self.named_parameters() if p.requires_grad]
        no_wd = [p for n, p in named if len(p.squeeze().shape) < 2 or n.endswith(".time_state")]
        wd = [p for n, p in named if len(p.squeeze().shape) >= 2 and not n.endswith(".time_state")]
        groups = []
        if no_wd:
            groups.append({"params": no_wd, "weight_decay": 0.0})
        if wd:
            groups.append({"params": wd, "weight_decay": float(getattr(self.args, "weight_decay", 0.0))})
        return groups

    # ---- forward path
    def adaptive_pooling(self, image_features):
        from . import fused
        if getattr(getattr(self, "args", None), "fused", False) and fused.visual_supported(image_features):
            osz = self.pool.output_size
            return fused.adaptive_pool(image_features, osz if isinstance(osz, int) else osz[0])
        B, Ln, D = image_features.shape
        side = int(Ln ** 0.5)
        x = image_features.view(B, side, side, D).permute(0, 3, 1, 2)
        return self.pool(x).view(B, D, -1).permute(0, 2, 1)

    def encode_images(self, images: dict, minibatch_size: int = None, normed: bool = True) -> torch.Tensor:
        """ViTs (frozen, no grad) in mini-batches of `minibatch_size` images -> pool -> projector
        (src/model.py:449-471; the reference's per-mini-batch torch.cuda.empty_cache() is a device sync
        plus an allocator flush and is deliberately not reproduced).  The reference encodes 4 images at a time to save
        memory; `args.vit_minibatch` raises that where the HBM allows (no activations are kept: the towers are frozen) --
        the tower GEMMs run at 0.6 PFLOP/s with 4 images (4 096 rows) and at 0.9 with 16."""
        if getattr(self, "vrwkv", None) is not None:         # v7.10 src/model.py:501-503: (features (B_img, L, C), ImageNet logits (B_img, 1000))
            return self.vrwkv(images["image"])
        if minibatch_size is None:
            minibatch_size = int(getattr(getattr(self, "args", None), "vit_minibatch", 4) or 4)
        keys = [k for k in ("dino", "siglip", "sam") if k in images]
        n = len(images[keys[0]])
        feats = []
        with torch.no_grad():
            for i in range(0, n, minibatch_size):
                feats.append(self.vit({k: images[k][i:i + minibatch_size] for k in keys}))
        image_features = feats[0] if len(feats) == 1 else torch.cat(feats, dim=0)
        # with a compressor every token of every image goes through the projector (v7.04 src/model.py:507-514: no 2-D pool)
        pooled = image_features.detach() if getattr(self, "vtc", None) is not None else self.adaptive_pooling(image_features.detach())
        if normed:
            return self.proj(pooled)
        return self.proj.pre_norm(pooled)               # ln_v is applied by the fused scatter

    def _images_per_sample(self, n_images, B):
        if B <= 0 or n_images % B != 0:
            raise ValueError(f"the compressor runs over all image tokens of a sample: {n_images} images do not divide among {B} samples")
        return n_images // B

    def compress_visual_tokens(self, image_features, reduction="pool"):
        """(B, N, L, D) projected image tokens -> the compressor over the N L tokens of each sample -> (B, N * num_token_per_image, D)
        (v7.04 src/model.py:516-529).  'pool': AdaptiveAvgPool1d over tokens; 'step': every (L // num_token_per_image)-th token."""
        if getattr(self, "vtc", None) is None:
            raise ValueError("compress_visual_tokens: the model has no compressor (build it with args.n_vtc_layer > 0)")
        if reduction not in ("pool", "step"):
            raise ValueError(f"reduction = {reduction!r}: 'pool' or 'step'")
        B, N, L, D = image_features.shape
        ntpi = int(self.args.num_token_per_image)
        if ntpi > L:
            raise ValueError(f"num_token_per_image = {ntpi} is more than the {L} tokens of an image: the compressor only reduces")
        return self.vtc(image_features.reshape(B, N * L, D), tail=(ntpi * N, reduction))

    def preparing_embedding(self, samples):
        """(input embeddings, labels); with args.modality_ffn a third entry, the image mask (B, T, 1) bool = input_ids == IMAGE_TOKEN_INDEX
        (v7.10 src/model.py:526).  With the RWKV vision encoder (args.n_vrwkv_layer) and images in the batch, the reference's 4-tuple
        (embeds, labels, mask, cls_logits) (src/model.py:505-526); mask is None without args.modality_ffn."""
        # called unbound, and `args` probed, because tests and the golden scripts call this method on stand-in objects that carry only
        # `rwkv`, `encode_images` and sometimes `args`
        modality = getattr(getattr(self, "args", None), "modality_ffn", 0)
        if getattr(self, "vrwkv", None) is not None and "images" in samples:
            x, labels, cls_logits = VisualRWKV._preparing_embedding_vrwkv(self, samples)
            return x, labels, ((samples["input_ids"] == IMAGE_TOKEN_INDEX).unsqueeze(-1) if modality else None), cls_logits
        res = VisualRWKV._preparing_embedding(self, samples)
        if modality:
            return (*res, (samples["input_ids"] == IMAGE_TOKEN_INDEX).unsqueeze(-1))
        return res

    @staticmethod
    def _placeholder_rows(selected, n_feat):
        """Row of the flattened token embeddings for each of n_feat feature rows, without a host synchronisation: the placeholders in order (a
        stable sort of the mask), -1 for the surplus when there are fewer placeholders than features (the reference keeps the first features and
        warns, src/model.py:519-523; the kernels drop a negative row both ways)."""
        n_tok = selected.numel()
        rows = torch.argsort(~selected, stable=True)
        if n_feat > n_tok:                              # more features than tokens at all: the surplus has no row
            rows = torch.cat((rows, rows.new_zeros(n_feat - n_tok)))
            ok = torch.arange(n_feat, device=rows.device) < n_tok
            return torch.where(ok & selected[rows], rows, torch.full_like(rows, -1)).contiguous()
        rows = rows[:n_feat]
        return torch.where(selected[rows], rows, torch.full_like(rows, -1)).contiguous()

    def _preparing_embedding_vrwkv(self, samples):
        """v7.10 src/model.py:505-526: every token of every image, from the RWKV vision encoder, into the placeholder rows.  Returns
        (embeds, labels, cls_logits)."""
        from . import fused
        ids = samples["input_ids"]
        B, Ln = ids.shape
        D = self.rwkv.emb.weight.shape[1]
        selected = ids.reshape(B * Ln) == IMAGE_TOKEN_INDEX
        pixels = samples["images"]["image"]
        if (getattr(self.args, "fused", False) and ids.is_cuda and self.rwkv.emb.weight.dtype == torch.bfloat16
                and not getattr(self.args, "check_image_tokens", True) and fused.vrwkv_supported(self.vrwkv, pixels)):
            # GPU path: ln_out of the encoder writes straight into the placeholder rows and forms the head's mean in the same pass
            L_img = (pixels.shape[-2] // self.args.patch_size) * (pixels.shape[-1] // self.args.patch_size)
            rows = VisualRWKV._placeholder_rows(selected, pixels.shape[0] * L_img)
            input_embeds = self.rwkv.emb(ids.reshape(B * Ln))    # not a view: the tail op writes into it and has a second output
            input_embeds, cls_logits = self.vrwkv(pixels, scatter=(input_embeds, rows))
            return input_embeds.view(B, Ln, D), samples["labels"], cls_logits
        image_features, cls_logits = self.encode_images(samples["images"])
        image_features = image_features.reshape(-1, image_features.shape[-1])
        input_embeds = self.rwkv.emb(ids).view(B * Ln, D)
        n_sel = int(selected.sum()) if getattr(self.args, "check_image_tokens", True) else image_features.shape[0]
        if n_sel != image_features.shape[0]:
            n_feat = image_features.shape[0]
            image_features = image_features[:n_sel]      # the reference truncates and warns (src/model.py:519-523)
            warnings.warn(f"image tokens: {n_sel}, but image features: {n_feat}")
        input_embeds = input_embeds.masked_scatter(selected[:, None], image_features.to(input_embeds.dtype))
        return input_embeds.view(B, Ln, D), samples["labels"], cls_logits

    def _cls_loss(self, loss, cls_logits, batch):
        """v7.10 src/model.py:489-492: the ImageNet classification loss of the vision encoder, added when the batch carries `cls_labels`."""
        if cls_logits is None or batch.get("cls_labels") is None:
            return loss
        cls_labels = batch["cls_labels"]
        if cls_logits.shape[0] != cls_labels.shape[0]:
            raise ValueError(f"cls_labels: {cls_labels.shape[0]} labels for {cls_logits.shape[0]} images -- the classification loss needs one image "
                             "per sample, as in the reference")
        return loss + F.cross_entropy(cls_logits, cls_labels)

    def _preparing_embedding(self, samples):
        if "images" not in samples:
            return self.rwkv.emb(samples["input_ids"]), samples["labels"]
        from . import fused
        ids = samples["input_ids"]
        B, Ln = ids.shape
        D = self.rwkv.emb.weight.shape[1]
        selected = ids.reshape(B * Ln) == IMAGE_TOKEN_INDEX
        vtc = getattr(self, "vtc", None)
        if (vtc is not None and getattr(self.args, "fused", False) and ids.is_cuda and self.rwkv.emb.weight.dtype == torch.bfloat16
                and not getattr(self.args, "check_image_tokens", True) and self.proj.ln_v.weight.dtype == torch.bfloat16
                and vtc.ln_out.weight.dtype == torch.bfloat16 and D % 64 == 0 and D <= 8192):
            # GPU path with a compressor: ln_v (one kernel: it feeds the compressor and cannot move into the scatter), the Blocks with their flips,
            # then ln_out + unpad + pool + scatter into the placeholder rows in one pass.  Same row list and surplus rule as below.
            pre = self.encode_images(samples["images"], normed=False)
            N = self._images_per_sample(pre.shape[0], B)
            ntpi = int(self.args.num_token_per_image)
            if ntpi > pre.shape[1]:
                raise ValueError(f"num_token_per_image = {ntpi} is more than the {pre.shape[1]} tokens of an image: the compressor only reduces")
            _, feats = fused.add_ln(pre.reshape(B, N * pre.shape[1], D), None, self.proj.ln_v)
            input_embeds = self.rwkv.emb(ids).view(B * Ln, D)
            n_feat = B * N * ntpi
            rows = torch.argsort(~selected, stable=True)
            if n_feat > B * Ln:                              # more features than tokens at all: the surplus has no row
                rows = torch.cat((rows, rows.new_zeros(n_feat - B * Ln)))
                ok = torch.arange(n_feat, device=rows.device) < B * Ln
                rows = torch.where(ok & selected[rows], rows, torch.full_like(rows, -1))
            else:
                rows = rows[:n_feat]
                rows = torch.where(selected[rows], rows, torch.full_like(rows, -1))
            input_embeds = vtc(feats, tail=(N * ntpi, "pool", input_embeds, rows.contiguous()))
            return input_embeds.view(B, Ln, D), samples["labels"]
        if vtc is not None:
            input_embeds = self.rwkv.emb(ids).view(B * Ln, D)
            image_features = self.encode_images(samples["images"])
            N = self._images_per_sample(image_features.shape[0], B)
            image_features = self.compress_visual_tokens(image_features.view(B, N, *image_features.shape[1:]))
            image_features = image_features.reshape(-1, image_features.shape[-1])
            n_sel = int(selected.sum())
            if n_sel != image_features.shape[0]:
                n_feat = image_features.shape[0]
                image_features = image_features[:n_sel]      # the reference truncates and warns (v7.04 src/model.py:546-550)
                warnings.warn(f"image tokens: {n_sel}, but image features: {n_feat}")
            input_embeds = input_embeds.masked_scatter(selected[:, None], image_features.to(input_embeds.dtype))
            return input_embeds.view(B, Ln, D), samples["labels"]
        if (getattr(self.args, "fused", False) and isinstance(getattr(self, "proj", None), MLPWithContextGating) and ids.is_cuda
                and self.rwkv.emb.weight.dtype == torch.bfloat16 and not getattr(self.args, "check_image_tokens", True)
                and self.proj.ln_v.weight.dtype == torch.bfloat16 and D % 64 == 0):
            # GPU path: ln_v of the projector writes straight into the placeholder rows (no masked_scatter, no host sync: the
            # row list comes from a stable sort of the mask).  The frozen towers run BEFORE the first trainable module is
            # touched, so the ZeRO-1 parameter all-gather of the previous step (dp.py) overlaps the ViT encode.
            feats = self.encode_images(samples["images"], normed=False)
            feats = feats.reshape(-1, feats.shape[-1])
            input_embeds = self.rwkv.emb(ids).view(B * Ln, D)
            n_feat = feats.shape[0]
            if n_feat > B * Ln:                              # more features than tokens at all: truncate like the reference
                feats, n_feat = feats[:B * Ln], B * Ln
            rows = torch.argsort(~selected, stable=True)[:n_feat]
            # fewer placeholders than features (a multi-image sample truncated at ctx_len): the reference keeps the first
            # n_sel features and warns (model.py:487-491).  Same result without a host synchronisation: the surplus
            # features get row -1, which the kernels drop in both directions -- they never overwrite text embeddings.
            rows = torch.where(selected[rows], rows, torch.full_like(rows, -1))
            input_embeds = fused.ln_scatter(input_embeds, feats, self.proj.ln_v, rows)
            return input_embeds.view(B, Ln, D), samples["labels"]
        input_embeds = self.rwkv.emb(ids)
        input_embeds = input_embeds.view(B * Ln, D)
        image_features = self.encode_images(samples["images"])
        image_features = image_features.view(-1, image_features.shape[-1])
        n_sel = int(selected.sum()) if getattr(self.args, "check_image_tokens", True) else image_features.shape[0]
        if n_sel != image_features.shape[0]:
            n_feat = image_features.shape[0]
            image_features = image_features[:n_sel]      # the reference truncates and warns (model.py:487-491)
            warnings.warn(f"image tokens: {n_sel}, but image features: {n_feat}")
        input_embeds = input_embeds.masked_scatter(selected[:, None], image_features.to(input_embeds.dtype))
        return input_embeds.view(B, Ln, D), samples["labels"]

    @staticmethod
    def packed_layout(samples, device):
        """The wkv7.PackedLayout of a batch from data.pack_batches (it carries `seg_lens`), or None for an ordinary padded batch."""
        if samples.get("seg_lens") is None:
            return None
        from .wkv7 import PackedLayout
        return PackedLayout(samples["seg_lens"], samples["input_ids"].shape[1], device, n_samples=samples.get("n_samples"))

    def forward(self, samples):
        """(logits, targets); with the RWKV vision encoder the reference's (logits, targets, cls_logits, cls_labels) (v7.10 src/model.py:467-471)."""
        x, targets, mk, cls_logits = _embed(self, samples)
        layout = self.packed_layout(samples, x.device)
        logits = self.rwkv(x, layout=layout, **mk) if layout is not None else self.rwkv(x, **mk)
        if getattr(self, "vrwkv", None) is not None:
            return logits, targets, cls_logits, samples.get("cls_labels")
        return logits, targets

    @staticmethod
    def loss_from_logits(logits, targets, layout=None, window=None):
        """Shifted CE, summed per sample over valid labels / max(valid,1), batch mean, wrapped in L2Wrap
        (src/model.py:418-434).  With a layout "sample" means segment of a packed row: the last row of a segment has no target, the mean
        runs over layout.n_samples; L2Wrap keeps the reference's formula on the packed (B, T) logits.
        window = (a, b) (train_step_cut): logits (B, b-a, V) are rows a .. b-1 of the (B, T) row `targets`; the result is their share of the
        row's loss -- row b-1 predicts token b, a row weighs 1 / (valid labels of its whole sample * B), L2Wrap's factor counts B * T."""
        if window is not None:
            if layout is not None:
                raise NotImplementedError("loss_from_logits: a window of a packed row")
            a, b = window
            B, T = targets.shape
            shift = torch.full_like(targets, IGNORE_INDEX)
            shift[:, :-1] = targets[:, 1:]
            valid = (shift != IGNORE_INDEX).sum(1).clamp(min=1)
            lab = shift[:, a:b].reshape(-1)
            loss = F.cross_entropy(logits.reshape(-1, logits.size(-1)), lab, ignore_index=IGNORE_INDEX, reduction="none")
            loss = (loss.view(B, b - a).sum(1) / valid).mean()
            return L2WrapWindow.apply(loss, logits, 1e-4 / (B * T))
        shift_logits = logits[..., :-1, :].contiguous()
        shift_labels = targets[..., 1:].contiguous()
        if layout is not None:
            Bp, Tp = targets.shape
            shift_labels = shift_labels.masked_fill(layout.first.view(Bp, Tp)[:, 1:].bool(), IGNORE_INDEX)
            seg = layout.seg_id[:, 1:].reshape(-1).long()        # the segment of the token a row predicts
            loss = F.cross_entropy(shift_logits.view(-1, shift_logits.size(-1)), shift_labels.view(-1),
                                   ignore_index=IGNORE_INDEX, reduction="none")
            total = torch.zeros(layout.n_segments, dtype=loss.dtype, device=loss.device).index_add_(0, seg, loss)
            valid = torch.zeros(layout.n_segments, dtype=loss.dtype, device=loss.device).index_add_(
                0, seg, (shift_labels.view(-1) != IGNORE_INDEX).to(loss.dtype))
            loss = (total / valid.clamp_min(1)).sum() / layout.n_samples
            return L2Wrap.apply(loss, logits)
        valid = (shift_labels != IGNORE_INDEX).sum(1)
        valid = torch.max(valid, torch.ones_like(valid))
        loss = F.cross_entropy(shift_logits.view(-1, shift_logits.size(-1)), shift_labels.view(-1),
                               ignore_index=IGNORE_INDEX, reduction="none")
        loss = (loss.view(shift_labels.size()).sum(1) / valid).mean()
        return L2Wrap.apply(loss, logits)

    def training_step(self, batch, batch_idx=0):
        """The language loss (loss_from_logits: L2Wrap on the language logits), plus the vision encoder's classification loss when the model has one
        and the batch carries `cls_labels` (v7.10 src/model.py:473-493), on every branch."""
        logits, cls = None, None
        if batch.get("seg_lens") is not None:            # a packed batch (data.pack_batches): per-segment state, shift and loss
            targets = batch["labels"]
            layout = self.packed_layout(batch, targets.device)
            if getattr(self.args, "fused", False):
                from . import fused
                if fused.head_loss_supported(self.rwkv.head, targets):
                    plan = fused.HeadPlan(targets, 0, IGNORE_INDEX, layout)     # head + loss on the labelled rows only, per-segment weights
                    x, _, mk, cls = _embed(self, batch)
                    h, _ = self.rwkv(x, hidden_only=True, layout=layout, **mk)
                    if fused.head_loss_supported(self.rwkv.head, targets, h):
                        return self._cls_loss(fused.head_loss(self.rwkv.head, h, plan), cls, batch)
                    return self._cls_loss(self.loss_from_logits(fused.linear(self.rwkv.head, h), targets, layout), cls, batch)
            logits, targets, *rest = self(batch)
            return self._cls_loss(self.loss_from_logits(logits, targets, layout), rest[0] if rest else None, batch)
        if getattr(self.args, "fused", False):
            from . import fused
            from .rwkv7 import CHUNK_LEN
            targets = batch["labels"]
            if fused.head_loss_supported(self.rwkv.head, targets):
                # head + loss as one node (backward dense on the labelled rows only); the labelled rows are counted before the forward is
                # issued, so that the head's backward finds the count in pinned memory without waiting
                plan = fused.HeadPlan(targets, (CHUNK_LEN - targets.shape[1] % CHUNK_LEN) % CHUNK_LEN, IGNORE_INDEX)
                x, _, mk, cls = _embed(self, batch)
                h, num_tokens_to_pad = self.rwkv(x, hidden_only=True, **mk)
                if num_tokens_to_pad == plan.pad and fused.head_loss_supported(self.rwkv.head, targets, h):
                    return self._cls_loss(fused.head_loss(self.rwkv.head, h, plan), cls, batch)
                logits = self.rwkv.unpad(fused.linear(self.rwkv.head, h), num_tokens_to_pad)     # RWKV.forward's head
        if logits is None:
            logits, targets, *rest = self(batch)
            cls = rest[0] if rest else None
        if getattr(self.args, "fused", False):
            from . import fused
            if fused.ce_supported(logits):
                return self._cls_loss(fused.loss_from_logits(logits, targets, IGNORE_INDEX), cls, batch)
        return self._cls_loss(self.loss_from_logits(logits, targets), cls, batch)

    def _segment_loss(self, h, targets, window):
        """The share of the row's loss that the hidden state h (B, b-a, C) of rows window = (a, b) carries (see loss_from_logits)."""
        if getattr(self.args, "fused", False):
            from . import fused
            if fused.head_loss_supported(self.rwkv.head, targets, h):
                return fused.head_loss(self.rwkv.head, h, fused.HeadPlan(targets, 0, IGNORE_INDEX, None, window))
            if h.is_cuda:
                return self.loss_from_logits(fused.linear(self.rwkv.head, h), targets, None, window)
        return self.loss_from_logits(self.rwkv.head(h), targets, None, window)

    def train_step_cut(self, batch, seg_len, truncate=False):
        """One training step on rows cut into segments of seg_len tokens: forward AND backward.  Gradients are left in `.grad`, the detached
        loss is returned.  Activation memory is that of one segment; what crosses a cut is a rwkv7.TrainCarry (two token rows and the WKV
        state per layer).
        Exact mode: the loss and the gradients of `training_step(batch).backward()` on the uncut rows, for one more forward pass --
        the segments run forward once without a graph to record the carry entering each; then, last segment first, each is run again
        from its carry with a graph, and its share of the loss and its outgoing carry (with the gradients the segment after it sent back)
        are back-propagated together.  The embedding (tokens, image features, projector) is formed once and back-propagated once.
        truncate=True: truncated back-propagation through time -- one pass, every segment starts from the detached carry of the one
        before: no gradient crosses a cut, nothing is recomputed."""
        if batch.get("seg_lens") is not None:
            raise NotImplementedError("train_step_cut: packed rows (a batch with seg_lens) cannot be cut")
        if getattr(self, "vrwkv", None) is not None:
            raise NotImplementedError("train_step_cut with args.n_vrwkv_layer is not built: the classification loss shares the vision encoder's graph "
                                      "with the embedding, which is back-propagated once at the end, and that joint backward has not been shown equal "
                                      "to training_step's; use training_step")
        if getattr(self, "vtc", None) is not None:
            raise NotImplementedError("train_step_cut with args.n_vtc_layer is not built: the compressor's rows are not cut; use training_step")
        if getattr(self.args, "modality_ffn", 0):
            raise NotImplementedError("train_step_cut with args.modality_ffn: cut rows are not routed (the carried channel-mix row would have to be "
                                      "re-normed per expert)")
        targets = batch["labels"]
        B, T = targets.shape
        seg_len = int(seg_len)
        if T % 16 != 0 or seg_len <= 0 or seg_len % 16 != 0:
            raise ValueError(f"train_step_cut: T ({T}) and seg_len ({seg_len}) must be multiples of 16")
        bounds = [(a, min(a + seg_len, T)) for a in range(0, T, seg_len)]
        n_layer = len(self.rwkv.blocks)
        from contextlib import nullcontext
        engine = next((p._vrwkv_engine() for p in self.parameters() if getattr(p, "_vrwkv_engine", None) is not None), None)      # dp.Zero1Engine
        with (engine.hold_reductions() if engine is not None else nullcontext()):
            x, _ = self.preparing_embedding(batch)
            xd = x.detach()
            gx = torch.zeros_like(xd) if x.requires_grad else None
            total = None

            def run(i, carry, want_grad):
                a, b = bounds[i]
                xs = xd[:, a:b].contiguous()
                if want_grad and gx is not None:
                    xs.requires_grad_(True)
                h, _, nxt = self.rwkv(xs, hidden_only=True, carry=carry)
                return xs, h, nxt

            if truncate:
                carry = TrainCarry(n_layer)
                for i, win in enumerate(bounds):
                    xs, h, nxt = run(i, carry, True)
                    loss = self._segment_loss(h, targets, win)
                    loss.backward()
                    if gx is not None:
                        gx[:, win[0]:win[1]] = xs.grad
                    total = loss.detach() if total is None else total + loss.detach()
                    carry = nxt.detach()
            else:
                carries = [TrainCarry(n_layer)]                          # the carry entering every segment
                with torch.no_grad():
                    for i in range(len(bounds) - 1):
                        carries.append(run(i, carries[-1], False)[2].detach())
                g_out = None                                             # gradients of the carry leaving segment i, from segment i + 1
                for i in reversed(range(len(bounds))):
                    cin = carries[i].detach(requires_grad=True) if i > 0 else carries[0]
                    xs, h, nxt = run(i, cin, True)
                    loss = self._segment_loss(h, targets, bounds[i])
                    roots, grads = [loss], [None]
                    if g_out is not None:
                        for t, g in zip(nxt.tensors(), g_out):
                            if g is not None and t.requires_grad:
                                roots.append(t)
                                grads.append(g.to(t.dtype))
                    torch.autograd.backward(roots, grads)
                    g_out = [t.grad for t in cin.tensors()] if i > 0 else None
                    if gx is not None:
                        gx[:, bounds[i][0]:bounds[i][1]] = xs.grad
                    total = loss.detach() if total is None else total + loss.detach()
                    carries[i] = None
                    del xs, h, nxt, loss, roots, grads, cin
            if gx is not None:
                x.backward(gx)
        return total

    @staticmethod
    def _sample_uniforms(max_new_tokens, B, generator, device):
        """Every u of a sampled call, drawn up front: (max_new_tokens, B) fp32 on `device`."""
        u = torch.rand(max_new_tokens, B, generator=generator, device=generator.device if generator is not None else "cpu")
        return u.to(device=device, dtype=torch.float32)

    @staticmethod
    def _stop_set(stop_token_idx):
        """stop_token_idx as the set of tokens that end a run: an int, or a sequence of ints (the applications stop on [0, 261])."""
        return frozenset(stop_token_idx) if isinstance(stop_token_idx, (list, tuple, set, frozenset)) else frozenset((stop_token_idx,))

    @staticmethod
    def _sampled_append(out, triple, done, stops):
        """One step's (token, logit, prob) rows into the result lists -- scalars for one row, lists of B values otherwise -- and whether
        the call is over: every row has produced a stop token."""
        tok, lg, pr = (t.tolist() for t in triple)
        for lst, v in zip(out, (tok, lg, pr)):
            lst.append(v[0] if len(v) == 1 else v)
        for b, t in enumerate(tok):
            done[b] = done[b] or t in stops
        return all(done)

    def _penalty_args(self, do_sample, temperature, top_p, presence_penalty, count_penalty, penalty_decay, token_ban):
        """The sampling arguments of generate / generate_stateful, checked; returns whether the call needs occurrence counts."""
        from . import sampling
        token_ban = tuple(token_ban)
        pen = sampling.penalised(presence_penalty, count_penalty, token_ban)
        if pen and not do_sample:
            raise ValueError("presence / count penalties and token_ban go with do_sample=True (the reference's applications sample; "
                             "top_p=0 is greedy decoding under them)")
        if do_sample:
            sampling.check_args(temperature, top_p, presence_penalty, count_penalty, penalty_decay, token_ban, self.rwkv.emb.weight.size(0))
        return pen

    @torch.no_grad()
    def generate(self, input_ids, images, do_sample, temperature, top_p, max_new_tokens, stop_token_idx, generator=None,
                 presence_penalty=0.0, count_penalty=0.0, penalty_decay=0.996, token_ban=()):
        """Decoding with the reference's semantics (src/model.py:496-530): the full sequence is re-run for every new token (stateful
        decoding is SURVEY.md 8f rank 1).  Greedy, or with do_sample the top-p / temperature pick of sampling.py on each step's last row
        (the reference raises there; its applications sample); generator: the torch.Generator of the call's uniform numbers.
        presence_penalty, count_penalty, penalty_decay, token_ban: the applications' loop around the pick (v7.10/app/app_gpu.py:56-86;
        sampling.py), do_sample only.  stop_token_idx: an int or a sequence of ints."""
        pen = self._penalty_args(do_sample, temperature, top_p, presence_penalty, count_penalty, penalty_decay, token_ban)
        stops = self._stop_set(stop_token_idx)
        samples = {"input_ids": input_ids, "images": images, "labels": torch.full_like(input_ids, IGNORE_INDEX)}
        if do_sample:
            from . import sampling
            x, _, mk, _ = _embed(self, samples)
            mk.pop("n_image", None)
            B = x.size(0)
            u_all = self._sample_uniforms(max_new_tokens, B, generator, x.device)
            out, done = ([], [], []), [False] * B
            occ = None
            for i in range(max_new_tokens):
                logits = self.rwkv(x, **mk)[:, -1, :].contiguous()
                nxt = torch.empty(B, 1, x.size(-1), device=x.device, dtype=x.dtype)
                if pen and occ is None:
                    occ = sampling.reset_occ(torch.empty(logits.shape, device=logits.device, dtype=torch.float32), token_ban)
                triple = sampling.pick(logits, temperature, top_p, u_all[i], self.rwkv.emb.weight.to(x.dtype), nxt,
                                       occ, presence_penalty, count_penalty, penalty_decay)
                if self._sampled_append(out, triple, done, stops):
                    break
                x = torch.cat((x, nxt), dim=-2)[:, -self.args.ctx_len:, :]
                if "mask" in mk:
                    mk["mask"] = torch.cat((mk["mask"], torch.zeros_like(mk["mask"][:, -1:])), dim=1)[:, -self.args.ctx_len:, :]
            return out
        x, _, mk, _ = _embed(self, samples)
        mk.pop("n_image", None)
        toks, lgs, prs = [], [], []
        for _ in range(max_new_tokens):
            logits = self.rwkv(x, **mk)[:, -1, :]
            nxt = torch.argmax(logits, dim=-1, keepdim=True)
            toks.append(nxt.item())
            lgs.append(logits.gather(-1, nxt).item())
            prs.append(torch.softmax(logits, dim=-1).gather(-1, nxt).item())
            if toks[-1] in stops:
                break
            x = torch.cat((x, self.rwkv.emb(nxt)), dim=-2)[:, -self.args.ctx_len:, :]
            if "mask" in mk:                                 # a generated token is text (v7.10 src/model.py:562-563)
                mk["mask"] = torch.cat((mk["mask"], torch.zeros_like(mk["mask"][:, -1:])), dim=1)[:, -self.args.ctx_len:, :]
        return toks, lgs, prs

    @torch.no_grad()
    def generate_stateful(self, input_ids, images, do_sample, temperature, top_p, max_new_tokens, stop_token_idx,
                          use_graph=None, generator=None, presence_penalty=0.0, count_penalty=0.0, penalty_decay=0.996, token_ban=()):
        """`generate` with the recurrent state carried between tokens: one prefill over the prompt, then one
        single-token step per new token (O(1) per token instead of re-running the whole sequence).
        The prompt is left-padded once, like `RWKV.forward` pads it (src/model.py:301-307), so the first token
        is the one `generate` returns; later tokens are conditioned on that same fixed prefix, whereas the
        reference's per-step re-padding changes the number of pad tokens as the sequence grows.
        do_sample: the pick of sampling.py instead of the argmax, with the call's uniform numbers drawn up front from `generator`.  Through
        the captured graph (bf16, fused, B <= 4) the pick is the step's last kernel and writes the next input itself: a token is one
        replay and one read-back; otherwise sampling.pick per token.  Several rows: every list entry holds B values, and the call ends
        when every row has produced a stop token (stop_token_idx: an int or a sequence of ints).
        presence_penalty, count_penalty, penalty_decay, token_ban (do_sample only): the occurrence counts live on the device beside the
        decoder, the graph's last kernel is the penalised pick (GraphDecoder(penalised=True)), and a token still costs one replay and one
        read-back; with all of them at their defaults the call is exactly the unpenalised one."""
        if getattr(self, "vrwkv", None) is not None:
            raise NotImplementedError("generate_stateful with args.n_vrwkv_layer: only the embedding differs, but the stateful path has not been "
                                      "shown equal to generate() with the vision encoder in front of it; use generate()")
        if getattr(self.args, "modality_ffn", 0):
            raise NotImplementedError("generate_stateful with args.modality_ffn: the state carries the channel-mix shift row as a LayerNorm output, and "
                                      "with two experts the next token needs that row under its own expert's LayerNorm (ln2 or ln_v), so the carried "
                                      "row would have to be re-normed per expert; use generate()")
        from .rwkv7 import CHUNK_LEN
        pen = self._penalty_args(do_sample, temperature, top_p, presence_penalty, count_penalty, penalty_decay, token_ban)
        stops = self._stop_set(stop_token_idx)
        samples = {"input_ids": input_ids, "images": images, "labels": torch.full_like(input_ids, IGNORE_INDEX)}
        x, _ = self.preparing_embedding(samples)
        x = x[:, -self.args.ctx_len:, :]
        rem = x.size(1) % CHUNK_LEN
        x = self.rwkv.pad_left(x, CHUNK_LEN - rem if rem else 0)
        logits, state = self.rwkv.forward_stateful(x, None, last_only=True)
        if use_graph is None:                            # captured step where the batched-GEMV decode path applies
            use_graph = (x.is_cuda and bool(getattr(self.args, "fused", False)) and x.dtype == torch.bfloat16 and x.size(0) <= 4
                         and max_new_tokens >= 8)
        if do_sample:
            return self._generate_stateful_sampled(logits, state, temperature, top_p, max_new_tokens, stops, use_graph, generator,
                                                   (presence_penalty, count_penalty, penalty_decay, tuple(token_ban)) if pen else None)
        decoder = self.rwkv.decoder_for(state) if use_graph and x.is_cuda else None     # one capture per batch size, re-used
        toks, lgs, prs = [], [], []
        for _ in range(max_new_tokens):
            nxt = torch.argmax(logits, dim=-1, keepdim=True)
            toks.append(nxt.item())
            lgs.append(logits.gather(-1, nxt).item())
            prs.append(torch.softmax(logits, dim=-1).gather(-1, nxt).item())
            if toks[-1] in stops or len(toks) == max_new_tokens:
                break
            if decoder is not None:
                logits = decoder(self.rwkv.emb(nxt))
            else:
                logits, state = self.rwkv.forward_stateful(self.rwkv.emb(nxt), state, last_only=True)
        return toks, lgs, prs

    def _generate_stateful_sampled(self, logits, state, temperature, top_p, max_new_tokens, stops, use_graph, generator, pen=None):
        """pen: None, or (presence, count, decay, token_ban) of a call that needs occurrence counts."""
        from . import sampling
        B = logits.size(0)
        presence, count, decay, token_ban = pen if pen is not None else (0.0, 0.0, 0.996, ())
        emb = self.rwkv.emb.weight
        u_all = self._sample_uniforms(max_new_tokens, B, generator, logits.device)
        logits = logits.contiguous()
        use_graph = bool(use_graph) and logits.is_cuda and sampling.kernel_supported(logits, emb)
        out, done = ([], [], []), [False] * B
        if use_graph:
            decoder = self.rwkv.decoder_for(state, sampled=True, penalised=pen is not None)
            decoder.pick.set(temperature, top_p, presence, count, decay)
            if pen is not None:
                decoder.pick.reset(token_ban)
            # the first token eagerly, from the prefill's logits, into the graph's input (and the graph's counts)
            triple = sampling.pick(logits, temperature, top_p, u_all[0], emb, decoder.x_in, decoder.pick.occ, presence, count, decay)
            for i in range(1, max_new_tokens + 1):
                if self._sampled_append(out, triple, done, stops) or i == max_new_tokens:
                    break
                triple = decoder.sample(u_all[i])
            return out
        nxt = torch.empty(B, 1, emb.size(1), device=logits.device, dtype=logits.dtype)
        occ = sampling.reset_occ(torch.empty(logits.shape, device=logits.device, dtype=torch.float32), token_ban) if pen is not None else None
        for i in range(max_new_tokens):
            triple = sampling.pick(logits, temperature, top_p, u_all[i], emb.to(logits.dtype), nxt, occ, presence, count, decay)
            if self._sampled_append(out, triple, done, stops) or i == max_new_tokens - 1:
                break
            logits, state = self.rwkv.forward_stateful(nxt, state, last_only=True)
            logits = logits.contiguous()
        return out
