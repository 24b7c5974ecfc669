"""Host-side mirrors of the reference's three model-forward call surfaces.

Each scorer keeps the argument names, order, dtypes and shapes of the reference entry point it
replaces, so the reference's predict drivers can call it unchanged:

* ``ZkScorer.__call__``      <- ``model_triple.model_attention_channel_e`` (code/imagebert_zk/model_triple.py:162-214;
                               fed by evaluate_normal.py:227-238) -> ``(loss, probs[B,2], [loss])``
* ``LdsScorer.__call__``     <- ``bertmodel(..., features, ...)`` (code/imagebert_lds/src/run_pretraining_predict_score.py:288-336)
                               -> ``next_sentence_prob[B,2]``
* ``LxmertScorer.forward``   <- ``KDDModel.forward`` (code/lxmert/src/tasks/kdd_model.py:183-214) -> ``(x_norm[B,768], None, logit[B,2])``
* ``KDDModel``               <- the same class as ``KDD`` drives it (kdd_model.py:28-43,54,131-152): no-argument constructor, ``.cuda()``,
                               ``.eval()``, ``state_dict()``, ``load_state_dict(sd, strict=False)``, ``model(...)``
* ``EnsembleScorer``         <- what ``code/main.py:41-59`` merges: the four members on the same pairs, one C call

All arithmetic of the forward runs in libmmscore (HIP, gfx950), including the de-duplication of the label-text tuples
(``dedup_labels=True`` hands the dense ``[B,10,8]`` ids to the library).  torch is used here only to own device buffers
and the stream.
Inputs may be numpy arrays or torch tensors (host or device); outputs follow the input kind.
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib as _lib
from .config import N_BOX, LABEL_LEN


def _is_np(x):
    return isinstance(x, np.ndarray) or not torch.is_tensor(x)


class _Base:
    def __init__(self, cfg, weights: dict, precision="auto", device: int = 0, chunk_pairs: int = 0,
                 stop_after: int = -1, dedup_labels: bool = True, pack_tokens: bool = True, fuse_layernorm="auto", fuse_attention="auto"):
        """precision: 1 / 2 / 3 / 4 (4 = fp8 weights and activations on the big encoder GEMMs, outside the
        1e-3 contract) or "auto" = ``weights.auto_precision``: 2 for bf16-representable matrices, 3 for a real fp32 checkpoint."""
        if not torch.cuda.is_available():
            raise _lib.MmsError("no HIP device visible: the scorers have no CPU path")
        if precision == "auto":
            from .weights import auto_precision
            precision = auto_precision(weights)
        if fuse_attention == "auto":
            # mms_config.fuse_attention = 2 (QKV projection + attention in one kernel, Q K^T / P V on split-bf16 MFMAs: the configuration bench.py measures; <= 4e-5
            # from the exact-fp32 attention at full depth, held to the oracle by tests/test_parity_gpu.py): zk / lds +5 % over the two-kernel route, lxmert +6.5 % since
            # round 5 (its 10-token box stream and BOTH directions of its cross-attention run in the fused kernel too: profiles/rd5*).  Precision mode 3 -- the mode
            # that follows an arbitrary fp32 checkpoint -- keeps the attention arithmetic exact (1: the same kernel with exact-fp32 attention MFMAs, bit-identical
            # to the two-kernel route; lxmert's cross-attention then stays on the two-kernel route): ADVICE r4.
            fuse_attention = 1 if precision == 3 else 2
        if fuse_layernorm == "auto":
            # mms_config.fuse_layernorm mask 3: bias + residual + LayerNorm in the epilogue of the attention-output and FFN-down projections of
            # the big launches (precision mode 2; gemm_pp_ln.h) -- no LayerNorm launches, no fp32 round trip of the pre-LayerNorm tensor;
            # +1.5 % on the bench batch (profiles/rd4b_*).  Other precision modes ignore it.
            fuse_layernorm = 3
        self.fuse_layernorm = 3 if fuse_layernorm is True else int(fuse_layernorm)
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self.dedup_labels = dedup_labels
        self.precision = precision
        self.fuse_attention = int(fuse_attention)      # what "auto" resolved to (bench.py reports it)
        self.handle = _lib.Handle(cfg, precision=precision, device=device, chunk_pairs=chunk_pairs, stop_after=stop_after,
                                  pack_tokens=pack_tokens, fuse_layernorm=fuse_layernorm, fuse_attention=fuse_attention)
        self.handle.load_weights(weights)
        self.logits = None

    # -- helpers ---------------------------------------------------------------------------------
    def _dev(self, x, dtype):
        t = torch.as_tensor(np.ascontiguousarray(x)) if _is_np(x) else x
        return t.to(device=self.device, dtype=dtype, non_blocking=True).contiguous()

    def _labels(self, label_ids, dtype):
        """[B,10,8] ids -> (dense ids, None, None): the library finds the distinct tuples itself; or, with
        ``dedup_labels=False``, (None, ids as [B*10,8], arange): every tuple is encoded, the dense reference graph."""
        lab = self._dev(label_ids, dtype).reshape(-1, LABEL_LEN)
        if self.dedup_labels:
            return lab, None, None
        return None, lab, torch.arange(lab.shape[0], device=self.device, dtype=torch.int32)

    def _run(self, struct, n, keep):
        logits = torch.empty((n, 2), device=self.device, dtype=torch.float32)
        probs = torch.empty((n, 2), device=self.device, dtype=torch.float32)
        st = torch.cuda.current_stream(self.device).cuda_stream
        if n > 0:
            self.handle.score(struct, logits.data_ptr(), probs.data_ptr(), st)
        self._keep = keep  # keep inputs alive until the stream has consumed them
        self.logits = logits
        return logits, probs

    def read_hidden(self, rows):
        """Debug: current hidden state (fp32 [rows,768]) of the last chunk."""
        out = torch.empty((rows, 768), device=self.device, dtype=torch.float32)
        self.handle.debug_read_x(out.data_ptr(), rows, torch.cuda.current_stream(self.device).cuda_stream)
        return out

    def close(self):
        self.handle.close()


class ZkScorer(_Base):
    def prepare(self, num_boxes, np_boxes_5, np_images_features, np_idx_class_labels, np_idx_query_, len_query_,
                labels, segment_ids=None):
        T = self.cfg.text_len
        q = self._dev(np_idx_query_, torch.int32)
        B = q.shape[0]
        if segment_ids is None:  # load_data_v4.py:204
            segment_ids = torch.tensor([0] * T + [1] * N_BOX, dtype=torch.int32).repeat(B, 1)
        dense, uniq, idx = self._labels(np_idx_class_labels, torch.int32)
        t = dict(num_boxes=self._dev(num_boxes, torch.int32), boxes=self._dev(np_boxes_5, torch.float32),
                 feats=self._dev(np_images_features, torch.float32), dense=dense, uniq=uniq, idx=idx, q=q,
                 lq=self._dev(len_query_, torch.int32), labels=self._dev(labels, torch.int64),
                 seg=self._dev(segment_ids, torch.int32))
        assert t["feats"].shape == (B, N_BOX, 2048) and t["boxes"].shape == (B, N_BOX, 5) and q.shape[1] == T
        s = _lib.ZkBatch(B, t["num_boxes"].data_ptr(), t["boxes"].data_ptr(), t["feats"].data_ptr(),
                         uniq.data_ptr() if uniq is not None else None, uniq.shape[0] if uniq is not None else 0,
                         idx.data_ptr() if idx is not None else None, q.data_ptr(), t["lq"].data_ptr(), t["labels"].data_ptr(),
                         t["seg"].data_ptr(), dense.data_ptr() if dense is not None else None)
        return s, B, t

    def score_prepared(self, prepared):
        s, B, keep = prepared
        return self._run(s, B, keep)

    def __call__(self, num_boxes, np_boxes_5, np_images_features, np_idx_class_labels, np_len_class_labels,
                 np_idx_query_, len_query_, labels, segment_ids=None, label_query=None, weight_label_query=None,
                 is_training=False, reuse=None):
        as_np = _is_np(np_images_features)
        prep = self.prepare(num_boxes, np_boxes_5, np_images_features, np_idx_class_labels, np_idx_query_,
                            len_query_, labels, segment_ids)
        logits, probs = self.score_prepared(prep)
        # mean softmax cross-entropy of the margin logits (model_triple.py:83,103) -- reported, unused at predict
        lab = prep[2]["labels"]
        loss = (torch.logsumexp(logits, 1) - logits.gather(1, lab[:, None]).squeeze(1)).mean()
        if as_np:
            return float(loss), probs.cpu().numpy(), [float(loss)]
        return loss, probs, [loss]


class LdsScorer(_Base):
    def prepare(self, features: dict):
        ids = self._dev(features["input_ids"], torch.int64)
        B = ids.shape[0]
        seg = features.get("segment_ids")
        seg = torch.zeros_like(ids) if seg is None else self._dev(seg, torch.int64)
        t = dict(ids=ids, seg=seg, feats=self._dev(features["features"], torch.float32),
                 lab=self._dev(features["labelfeat"], torch.int64))
        assert t["feats"].shape == (B, N_BOX, 2048) and t["lab"].shape == (B, N_BOX, LABEL_LEN)
        s = _lib.LdsBatch(B, ids.data_ptr(), seg.data_ptr(), t["feats"].data_ptr(), t["lab"].data_ptr())
        return s, B, t

    def score_prepared(self, prepared):
        s, B, keep = prepared
        return self._run(s, B, keep)

    def __call__(self, features: dict, **_ignored):
        as_np = _is_np(features["features"])
        _, probs = self.score_prepared(self.prepare(features))
        return probs.cpu().numpy() if as_np else probs


class LxmertScorer(_Base):
    def prepare(self, input_ids, boxes_label_input_ids, input_mask, feats, boxes, visual_attention_mask, want_x_norm=False):
        ids = self._dev(input_ids, torch.int64)
        B = ids.shape[0]
        if input_mask is None:  # modeling.py:878-879
            input_mask = torch.ones_like(ids)
        if visual_attention_mask is None:
            visual_attention_mask = torch.ones((B, N_BOX), dtype=torch.float32)
        dense, uniq, idx = self._labels(boxes_label_input_ids, torch.int64)
        t = dict(ids=ids, mask=self._dev(input_mask, torch.int64), dense=dense, uniq=uniq, idx=idx,
                 feats=self._dev(feats, torch.float32), boxes=self._dev(boxes, torch.float32),
                 vm=self._dev(visual_attention_mask, torch.float32))
        if want_x_norm:
            t["x_norm"] = torch.empty((B, 768), device=self.device, dtype=torch.float32)
        assert t["feats"].shape == (B, N_BOX, 2048) and t["boxes"].shape == (B, N_BOX, 4)
        s = _lib.LxmertBatch(B, ids.data_ptr(), t["mask"].data_ptr(), uniq.data_ptr() if uniq is not None else None,
                             uniq.shape[0] if uniq is not None else 0, idx.data_ptr() if idx is not None else None,
                             t["feats"].data_ptr(), t["boxes"].data_ptr(), t["vm"].data_ptr(),
                             dense.data_ptr() if dense is not None else None,
                             t["x_norm"].data_ptr() if want_x_norm and B > 0 else None)
        return s, B, t

    def score_prepared(self, prepared):
        s, B, keep = prepared
        return self._run(s, B, keep)

    def forward(self, input_ids, boxes_label_input_ids, segment_ids, input_mask, boxes_label_segment_ids,
                boxes_label_input_mask, feats, boxes, visual_attention_mask):
        """Same positional signature and return tuple as KDDModel.forward: ``(x_norm, lang_prediction_scores, logit)``
        with x_norm = pooled / max(||pooled||, 1e-12) (kdd_model.py:204-205).  segment ids are all-zero in the reference
        feed (kdd_model.py:97-100 passes None) and the label mask is computed but unused there (modeling.py:579,900-902);
        the MLM head's output (kdd_model.py:201-202) is discarded by every caller and is not computed: None."""
        as_np = _is_np(feats)
        prep = self.prepare(input_ids, boxes_label_input_ids, input_mask, feats, boxes, visual_attention_mask, want_x_norm=True)
        logits, _ = self.score_prepared(prep)
        x_norm = prep[2]["x_norm"]
        return (x_norm.cpu().numpy() if as_np else x_norm, None, logits.cpu().numpy() if as_np else logits)

    __call__ = forward


class KDDModel(torch.nn.Module):
    """``tasks.kdd_model.KDDModel`` as its callers use it (code/lxmert/src/tasks/kdd_model.py:25-60,86-103,131-152): built with no
    arguments, ``.cuda()`` / ``.to()`` / ``.eval()`` return the module, ``state_dict()`` lists the reference's tensors (470 at full size:
    ``weights.kdd_state_dict_shapes``), ``load_state_dict(sd, strict=False)`` takes a ``torch.load('BEST.pth')`` (``module.`` prefixes of a
    DataParallel save accepted) and ``model(...)`` is the 9-argument ``KDDModel.forward`` -> ``(x_norm, None, logit)``.

    An ``nn.Module`` without parameters: the tensors live on the host as the checkpoint holds them (fp32) and, once a forward needs them,
    inside one ``mms_handle`` (``LxmertScorer``); a ``load_state_dict`` after that re-creates the handle at the next forward.  A fresh
    instance holds this repo's seeded synthetic weights (the reference: ``init_bert_weights`` noise, kdd_model.py:172) -- every real use
    loads a checkpoint next (``KDD.__init__`` -> ``self.load(args.load)``, :36-37).  ``logit_W`` and the MLM heads ``cls.*`` are carried
    for the round trip and never reach the device: the predict path reads ``logit_fc`` (``task_amsloss`` off, :207-212), and
    ``lang_prediction_scores`` is discarded by every caller.  Inference only: ``train(True)`` raises; there is no CPU forward."""

    def __init__(self, cfg=None, weights=None, device=None, **scorer_kw):
        super().__init__()
        from .config import LxmertConfig
        self.cfg = cfg if cfg is not None else LxmertConfig()        # args.llayers / xlayers / rlayers = 9 / 5 / 5 (param.py:72-74)
        self.config = self.cfg                                       # kdd_model.py:164
        self.training = False
        self._scorer_kw = scorer_kw
        self._device = device                                        # None until .cuda() / .to() or the first forward picks one
        self._host = None                                            # {name: np.float32 array}: the checkpoint as loaded
        self._scorer = None
        self._stale = True
        if weights is not None:
            self.load_state_dict(weights, strict=False)

    # -- host-side tensors -----------------------------------------------------------------------
    def _tensors(self):
        if self._host is None:
            from . import weights as W
            shapes = W.kdd_state_dict_shapes(self.cfg)
            host = {k: np.array(v) for k, v in W.make_weights(self.cfg).items()}      # private, writeable copies of the memoised arrays
            for k, shp in shapes.items():
                if k not in host:
                    host[k] = W.normal("kdd/" + k, shp, 20200823, std=0.02) if k == "logit_W" else np.zeros(shp, np.float32)
            host["cls.predictions.decoder.weight"] = host["lxrt_encoder.model.bert.embeddings.word_embeddings.weight"]   # tied
            self._host = {k: host[k] for k in shapes}
        return self._host

    def state_dict(self, destination=None, prefix="", keep_vars=False):
        import collections
        out = collections.OrderedDict() if destination is None else destination
        for k, v in self._tensors().items():
            out[prefix + k] = torch.from_numpy(v)                    # shares the host copy, like Module.state_dict(); the DEVICE copy follows
        return out                                                   # load_state_dict only -- in-place edits of these tensors do not reach it

    def load_state_dict(self, state_dict, strict=True, assign=False):
        from . import weights as W
        from torch.nn.modules.module import _IncompatibleKeys
        shapes = W.kdd_state_dict_shapes(self.cfg)
        got, unexpected, errors = {}, [], []
        for k, v in state_dict.items():
            name = k[7:] if k.startswith("module.") else k
            if name not in shapes:
                unexpected.append(k)
                continue
            a = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            if tuple(a.shape) != tuple(shapes[name]):
                errors.append("size mismatch for %s: copying a param with shape %s from checkpoint, the shape in current model is %s."
                              % (name, tuple(a.shape), tuple(shapes[name])))
                continue
            got[name] = np.array(a, dtype=np.float32, order="C")     # a private copy, like Module.load_state_dict's copy_
        missing = [k for k in shapes if k not in got]
        if strict and (missing or unexpected):
            errors.insert(0, "Missing key(s) in state_dict: %s. Unexpected key(s) in state_dict: %s." % (missing[:8], unexpected[:8]))
        if errors:
            raise RuntimeError("Error(s) in loading state_dict for KDDModel:\n\t" + "\n\t".join(errors))
        if got:
            host = dict(self._tensors())
            host.update(got)
            self._host = host
            self._stale = True
        return _IncompatibleKeys(missing, unexpected)

    # -- nn.Module protocol the reference's driver touches ---------------------------------------
    def train(self, mode: bool = True):
        if mode:
            raise _lib.MmsError("KDDModel drop-in is inference only (kdd_model.py:54 calls .eval())")
        self.training = False
        return self

    def cuda(self, device=None):
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        return self._place(torch.device("cuda", device) if isinstance(device, int) else torch.device(device))

    def to(self, *args, **kwargs):
        dev = kwargs.get("device", next((a for a in args if isinstance(a, (str, torch.device, int))), None))
        if dev is None:
            return self                                              # dtype-only moves: the arithmetic is the library's, nothing to cast
        return self._place(torch.device(dev) if not isinstance(dev, int) else torch.device("cuda", dev))

    def cpu(self):
        raise _lib.MmsError("KDDModel drop-in has no CPU forward (the reference's CPU path is what oracle/ restates)")

    def _place(self, dev):
        if dev.type != "cuda":
            return self.cpu()
        idx = dev.index if dev.index is not None else 0
        if self._device != idx:
            self._device, self._stale = idx, True
        return self

    def _live(self):
        if self._scorer is None or self._stale:
            from . import weights as W
            if self._scorer is not None:
                self._scorer.close()
            used = W.expected_shapes(self.cfg)
            t = self._tensors()
            self._scorer = LxmertScorer(self.cfg, {k: t[k] for k in used}, device=self._device or 0, **self._scorer_kw)
            self._stale = False
        return self._scorer

    def forward(self, input_ids, boxes_label_input_ids, segment_ids, input_mask, boxes_label_segment_ids,
                boxes_label_input_mask, feats, boxes, visual_attention_mask):
        return self._live().forward(input_ids, boxes_label_input_ids, segment_ids, input_mask, boxes_label_segment_ids,
                                    boxes_label_input_mask, feats, boxes, visual_attention_mask)

    def close(self):
        if self._scorer is not None:
            self._scorer.close()
            self._scorer = None
            self._stale = True


KDDModelDropIn = KDDModel


class EnsembleScorer:
    """The four members code/main.py:41-59 merges -- zk on the query, zk on its sen2forest rewrite, lds, lxmert -- on the SAME
    pairs in ONE library call (``mms_score_ensemble``, BASELINE.json config 5): box features split once per launch wave, label
    tuples de-duplicated once, zk's image-token stage run once for both query variants, merged score
    ``0.2*zk + 0.2*zk_s2f + 0.3*lds + 0.3*lxmert`` computed on the device so that the exchange step stays one fp32 per pair."""

    WEIGHTS = (0.2, 0.2, 0.3, 0.3)   # main.py:59

    def __init__(self, zk: "ZkScorer", lds: "LdsScorer", lxmert: "LxmertScorer", weights=WEIGHTS):
        self.zk, self.lds, self.lxmert = zk, lds, lxmert
        self.device = zk.device
        self.set_weights(weights)
        self.lib = _lib.load()

    def set_weights(self, w):
        """The four merge weights of the following calls (zk, zk on the sen2forest rewrite, lds, lxmert) -- e.g. ``ensemble.fit_weights``'s winner
        on the valid set instead of main.py:59's constants."""
        w = tuple(float(x) for x in w)
        if len(w) != 4:
            raise ValueError("the ensemble merges four members, not %d" % len(w))
        self.weights = w
        self.w = (_lib.C.c_float * 4)(*w)

    def prepare(self, feed: dict):
        """feed keys (numpy or torch, any integer dtype): feats [B,10,2048], boxes_5 [B,10,5], num_boxes [B], label_ids
        [B,10,8], query_ids / s2f_query_ids [B,20], len_query / s2f_len_query [B], labels [B], lx_input_ids /
        lx_input_mask [B,23]."""
        d = self.zk._dev
        i32 = torch.int32
        t = dict(feats=d(feed["feats"], torch.float32), boxes=d(feed["boxes_5"], torch.float32), nb=d(feed["num_boxes"], i32),
                 lab=d(feed["label_ids"], i32), q=d(feed["query_ids"], i32), lq=d(feed["len_query"], i32),
                 q2=d(feed["s2f_query_ids"], i32), lq2=d(feed["s2f_len_query"], i32), labels=d(feed["labels"], torch.int64),
                 lx=d(feed["lx_input_ids"], i32), lxm=d(feed["lx_input_mask"], i32))
        B = t["q"].shape[0]
        assert t["feats"].shape == (B, N_BOX, 2048) and t["boxes"].shape == (B, N_BOX, 5) and t["lab"].shape == (B, N_BOX, LABEL_LEN)
        assert t["q"].shape[1] == self.zk.cfg.text_len == self.lds.cfg.text_len and t["lx"].shape[1] == self.lxmert.cfg.text_len
        s = _lib.EnsembleBatch(B, t["feats"].data_ptr(), t["boxes"].data_ptr(), t["nb"].data_ptr(), t["lab"].data_ptr(),
                               t["q"].data_ptr(), t["lq"].data_ptr(), t["q2"].data_ptr(), t["lq2"].data_ptr(),
                               t["labels"].data_ptr(), t["lx"].data_ptr(), t["lxm"].data_ptr())
        return s, B, t

    def score_prepared(self, prepared, members: bool = True, cascade=None, plan=None):
        """-> (merged [B], member scores [4,B] or None), device fp32.
        ``plan=(group_ids, stages)``: the plan form (``mms_score_ensemble_plan``, include/mmscore.h) -- ``stages`` as ``ensemble.plan`` takes them,
        ``group_ids`` [B] the query id of each pair (``None`` for a one-stage plan) -- -> (merged, members, reached [B] uint8: the stages each pair
        went through); ``self.last_scored`` = the pairs each stage scored.  A member that was not computed for a pair is exactly +0.0.
        ``cascade=(group_ids, keep)``: the cascade form (``mms_score_ensemble_cascade``, include/mmscore.h) -- lxmert scores every pair, the best
        ``keep`` pairs of each query (``group_ids`` [B]: the query id of each pair) go through the other three members, a pruned pair's members
        0-2 are exact zeros -- -> (merged, members, kept [B] bool); ``self.last_kept`` = the number of kept pairs."""
        if plan is not None and cascade is not None:
            raise ValueError("plan= and cascade= are two forms of one call: give one")
        s, B, keep = prepared
        merged = torch.empty((B,), device=self.device, dtype=torch.float32)
        mem = torch.empty((4, B), device=self.device, dtype=torch.float32) if members else None
        if plan is not None:
            from . import ensemble as _ens
            group_ids, stages = plan
            stages = _ens.plan(stages)
            _ens._plan_weights(stages, self.weights)
            if group_ids is None and len(stages) > 1:
                raise ValueError("plan: only a one-stage plan may leave the group ids out")
            gid = None
            if group_ids is not None:
                gid = self.zk._dev(group_ids, torch.int64)
                if gid.shape != (B,):
                    raise ValueError("plan: group_ids must hold one query id per pair")
            rec = (_lib.PlanStage * len(stages))(*[_lib.PlanStage(m, k, sk, 0) for m, k, sk in stages])
            reached = torch.zeros((B,), device=self.device, dtype=torch.uint8)
            scored = (_lib.C.c_int64 * len(stages))()
            if B > 0:
                st = torch.cuda.current_stream(self.device).cuda_stream
                rc = self.lib.mms_score_ensemble_plan(self.zk.handle._h, self.lds.handle._h, self.lxmert.handle._h, _lib.C.byref(s),
                                                      gid.data_ptr() if gid is not None else None, rec, len(stages), self.w, merged.data_ptr(),
                                                      mem.data_ptr() if members else None, reached.data_ptr(), scored, st)
                if rc != 0:
                    raise _lib.MmsError("mms_score_ensemble_plan failed (%d): %s" % (rc, self.lib.mms_last_error(self.zk.handle._h).decode()))
            self._keep = (keep, gid)
            self.last_scored = [int(v) for v in scored]
            return merged, mem, reached
        if cascade is not None:
            group_ids, n_keep = cascade
            gid = self.zk._dev(group_ids, torch.int64)
            if gid.shape != (B,):
                raise ValueError("cascade: group_ids must hold one query id per pair")
            kept = torch.empty((B,), device=self.device, dtype=torch.uint8)
            nk = _lib.C.c_int64(0)
            if B > 0:
                st = torch.cuda.current_stream(self.device).cuda_stream
                rc = self.lib.mms_score_ensemble_cascade(self.zk.handle._h, self.lds.handle._h, self.lxmert.handle._h, _lib.C.byref(s), gid.data_ptr(),
                                                         int(n_keep), self.w, merged.data_ptr(), mem.data_ptr() if members else None,
                                                         kept.data_ptr(), _lib.C.byref(nk), st)
                if rc != 0:
                    raise _lib.MmsError("mms_score_ensemble_cascade failed (%d): %s" % (rc, self.lib.mms_last_error(self.zk.handle._h).decode()))
            self._keep = (keep, gid)
            self.last_kept = int(nk.value)
            return merged, mem, kept.bool()
        if B > 0:
            st = torch.cuda.current_stream(self.device).cuda_stream
            rc = self.lib.mms_score_ensemble(self.zk.handle._h, self.lds.handle._h, self.lxmert.handle._h, _lib.C.byref(s), self.w,
                                             merged.data_ptr(), mem.data_ptr() if members else None, st)
            if rc != 0:
                raise _lib.MmsError("mms_score_ensemble failed (%d): %s" % (rc, self.lib.mms_last_error(self.zk.handle._h).decode()))
        self._keep = keep
        return merged, mem

    def __call__(self, feed: dict, members: bool = True, cascade=None, plan=None):
        if plan is not None and cascade is not None:
            raise ValueError("plan= and cascade= are two forms of one call: give one")
        return self.score_prepared(self.prepare(feed), members, cascade, plan)

    def close(self):
        for m in (self.zk, self.lds, self.lxmert):
            m.close()


def make_scorer(cfg, weights, **kw):
    return {"zk": ZkScorer, "lds": LdsScorer, "lxmert": LxmertScorer}[cfg.name](cfg, weights, **kw)


def score_batch(scorer, batch: dict):
    """Run a synth.*_batch dict through the matching scorer; returns (logits, probs) device tensors."""
    n = scorer.cfg.name
    if n == "zk":
        p = scorer.prepare(batch["num_boxes"], batch["np_boxes_5"], batch["np_images_features"], batch["np_idx_class_labels"],
                           batch["np_idx_query_"], batch["len_query_"], batch["labels"], batch["segment_ids"])
    elif n == "lds":
        p = scorer.prepare(batch)
    else:
        p = scorer.prepare(batch["input_ids"], batch["boxes_label_input_ids"], batch["input_mask"], batch["feats"],
                           batch["boxes"], batch["visual_attention_mask"])
    return scorer.score_prepared(p)
