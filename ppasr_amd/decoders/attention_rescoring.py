"""Attention rescoring of CTC n-best lists with the checkpoint's own attention decoder (``decoder.left_decoder.*`` /
``decoder.right_decoder.*``, the reference's ``BiTransformerDecoder``), on the HIP kernels behind ``ppasr_rescore``.

The reference trains this decoder with every Conformer-family model and never calls it at inference; the decode mode is
WeNet's ``attention_rescoring``: n-best of the CTC prefix beam search -> score each hypothesis with the left and right
decoder over the encoder output -> add the CTC score -> best.
"""
import ctypes

import numpy as np
import torch

from ppasr_amd import _lib
from ppasr_amd.decoders.beam_search_decoder import _text, beam_search_ids

__all__ = ["AttentionRescorer", "attention_rescoring", "MAX_ROWS"]

MAX_ROWS = 256  # rows per hypothesis (tokens + 1) the kernels are built for


class AttentionRescorer:
    """``state_dict``: the Paddle-layout checkpoint (only its ``decoder.*`` entries are read); ``decoder_conf``: the
    section of the reference YAML (attention_heads, linear_units, num_blocks, r_num_blocks; dropout keys are accepted and
    ignored).  Anything the kernels are not built for is refused at construction (``PPASR_EUNSUPPORTED``), a checkpoint
    without the decoder's weights with ``PPASR_EMISSING``."""

    _IGNORED = ("dropout_rate", "positional_dropout_rate", "self_attention_dropout_rate", "src_attention_dropout_rate")

    def __init__(self, state_dict, vocab_size, decoder_conf=None, device="cuda:0", d_model=256, max_len=5000):
        if not torch.cuda.is_available():
            raise _lib.PPASRHipError("no HIP device visible: ppasr_amd has no CPU fallback")
        conf = dict(decoder_conf or {})
        for k in self._IGNORED:
            conf.pop(k, None)
        if not conf.pop("normalize_before", True):
            raise _lib.PPASRHipError("attention decoder: normalize_before = False is not built", _lib.PPASR_EUNSUPPORTED)
        if conf.pop("concat_after", False):
            raise _lib.PPASRHipError("attention decoder: concat_after = True is not built", _lib.PPASR_EUNSUPPORTED)
        if conf.pop("input_layer", "embed") != "embed" or not conf.pop("use_output_layer", True):
            raise ValueError("attention decoder: input_layer 'embed' with an output layer only")  # decoder.py:171
        self.heads = int(conf.pop("attention_heads", 4))
        self.linear_units = int(conf.pop("linear_units", 2048))
        self.num_blocks = int(conf.pop("num_blocks", 6))
        self.r_num_blocks = int(conf.pop("r_num_blocks", 0))
        max_len = int(conf.pop("max_len", max_len))
        self.max_len = max_len if max_len > 0 else 5000  # (0: the library's default table length)
        if conf:
            raise ValueError("unknown decoder_conf keys: " + ", ".join(sorted(conf)))
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.vocab_size = int(vocab_size)
        self.d_model = int(d_model)
        sd = {k: v for k, v in state_dict.items() if k.startswith("decoder.")}
        if not sd:  # (the library names the first weight it misses)
            sd = {"__none__": np.zeros(1, np.float32)}
        keep = []
        blobs = (_lib.WeightBlob * len(sd))()
        for i, (name, arr) in enumerate(sd.items()):
            a = np.ascontiguousarray(arr, dtype=np.float32)
            keep.append(a)
            blobs[i].name = name.encode()
            blobs[i].data_host = a.ctypes.data
            blobs[i].ndim = a.ndim
            for j in range(a.ndim):
                blobs[i].shape[j] = a.shape[j]
        desc = _lib.RescorerDesc(self.vocab_size, self.d_model, self.heads, self.linear_units, self.num_blocks,
                                 self.r_num_blocks, max_len)
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ppasr_rescorer_create(ctypes.byref(desc), blobs, len(sd), ctypes.byref(handle)))
        self._h = handle
        self._ws = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self.lib.ppasr_rescorer_destroy(h)
            self._h = None

    def _workspace(self, B, Tp, nbest, max_tokens):
        need = int(self.lib.ppasr_rescorer_workspace_bytes(self._h, B, Tp, nbest, max_tokens))
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        return ws

    def rescore(self, memory, out_lens, tokens, lens, ctc_scores, ctc_weight=0.5, reverse_weight=0.0,
                return_token_logp=False, return_logits=False, workspace=None, out=None):
        """memory [B, Tp, D] f32, out_lens [B] i32 or None, tokens [B, nbest, max_tokens] i32, lens [B, nbest] i32,
        ctc_scores [B, nbest] f64 (the outputs of ``beam_search_ids``) -> dict of device tensors: att, r_att, total
        [B, nbest] f64, best [B] i32 (+ token_logp [B, nbest, 2, max_tokens + 1], logits [.., V] when asked for).
        Asynchronous on the current stream.  ``workspace`` / ``out``: caller-owned buffers (tests)."""
        dev = self.device
        memory = torch.as_tensor(memory, dtype=torch.float32).to(dev).contiguous()
        tokens = torch.as_tensor(tokens, dtype=torch.int32).to(dev).contiguous()
        lens = torch.as_tensor(lens, dtype=torch.int32).to(dev).contiguous()
        ctc_scores = torch.as_tensor(ctc_scores, dtype=torch.float64).to(dev).contiguous()
        ol = None if out_lens is None else torch.as_tensor(out_lens, dtype=torch.int32).to(dev).contiguous()
        B, Tp, D = memory.shape
        _, nbest, mt = tokens.shape
        assert D == self.d_model and lens.shape == (B, nbest) and ctc_scores.shape == (B, nbest)
        o = {} if out is None else out
        new = lambda name, shape, dt: o[name] if name in o else torch.empty(shape, dtype=dt, device=dev)
        res = dict(att=new("att", (B, nbest), torch.float64), r_att=new("r_att", (B, nbest), torch.float64),
                   total=new("total", (B, nbest), torch.float64), best=new("best", (B,), torch.int32))
        if return_token_logp:
            res["token_logp"] = new("token_logp", (B, nbest, 2, mt + 1), torch.float32)
        if return_logits:
            res["logits"] = new("logits", (B, nbest, 2, mt + 1, self.vocab_size), torch.float32)
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(dev):
            ws = workspace if workspace is not None else self._workspace(B, Tp, nbest, mt)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(self.lib.ppasr_rescore(self._h, memory.data_ptr(), ptr(ol), B, Tp, ptr(tokens) if mt else None,
                                              lens.data_ptr(), ctc_scores.data_ptr(), nbest, mt, float(ctc_weight),
                                              float(reverse_weight), res["att"].data_ptr(), res["r_att"].data_ptr(),
                                              res["total"].data_ptr(), res["best"].data_ptr(), ptr(res.get("token_logp")),
                                              ptr(res.get("logits")), ws.data_ptr(), ws.numel(), stream))
        return res

    def default_max_steps(self, Tp):
        """WeNet's ``maxlen = T'``, within what the kernels and the positional table take."""
        return max(1, min(int(Tp), MAX_ROWS - 1, self.max_len - 1))

    def decode_workspace_bytes(self, B, Tp, beam_size, max_steps, joint=False):
        fn = self.lib.ppasr_attention_decode_joint_workspace_bytes if joint else self.lib.ppasr_attention_decode_workspace_bytes
        return int(fn(self._h, B, Tp, beam_size, max_steps))

    def decode(self, memory, out_lens, beam_size=10, max_steps=None, return_token_logp=False, return_trace=False,
               workspace=None, out=None, ctc_probs=None, ctc_weight=0.0, blank=0):
        """Attention beam search with the left decoder (``ppasr_attention_decode``; the semantics are the header comment
        of ``csrc/attn_decode.hip``): memory [B, Tp, D] f32, out_lens [B] i32 or None -> dict of device tensors: tokens
        [B, beam_size, max_steps] i32 (-1 behind the hypothesis), lens [B, beam_size] i32, scores [B, beam_size] f64 (best
        first), ended [B, beam_size] i32, steps_run [1] i32 (+ token_logp [B, beam_size, max_steps + 1] f32; trace_parent,
        trace_token i32 and trace_score f64 [max_steps, B, beam_size] when asked for).  ``max_steps=None``:
        ``min(Tp, 255, max_len - 1)``.  Asynchronous on the current stream, nothing is read back.  ``workspace`` / ``out``:
        caller-owned buffers (tests).

        ``ctc_probs`` [B, Tp, V] f32 (the CTC head's softmax output of the same encode), ``ctc_weight`` and ``blank``
        select the CTC-joint search (``ppasr_attention_decode_joint``, semantics: the header comment of
        ``csrc/attn_decode_joint.hip``): every candidate also gets ``ctc_weight`` x its CTC prefix score.  Then the beam may
        hold rows at -inf (lens 0), token_logp holds the attention summands, and token_ctc [B, beam_size, max_steps + 1]
        f32 / trace_ctc [max_steps, B, beam_size] f32 come with token_logp / the trace.  With ``ctc_probs=None`` and
        ``ctc_weight=0`` (the defaults) the plain entry point runs, as before."""
        dev = self.device
        memory = torch.as_tensor(memory, dtype=torch.float32).to(dev).contiguous()
        ol = None if out_lens is None else torch.as_tensor(out_lens, dtype=torch.int32).to(dev).contiguous()
        B, Tp, D = memory.shape
        assert D == self.d_model and (ol is None or ol.shape == (B,))
        N = int(beam_size)
        P = self.default_max_steps(Tp) if max_steps is None else int(max_steps)
        o = {} if out is None else out
        new = lambda name, shape, dt: o[name] if name in o else torch.empty(shape, dtype=dt, device=dev)
        shp = lambda *s: tuple(max(int(v), 0) for v in s)
        res = dict(tokens=new("tokens", shp(B, N, P), torch.int32), lens=new("lens", shp(B, N), torch.int32),
                   scores=new("scores", shp(B, N), torch.float64), ended=new("ended", shp(B, N), torch.int32),
                   steps_run=new("steps_run", (1,), torch.int32))
        if return_token_logp:
            res["token_logp"] = new("token_logp", shp(B, N, P + 1), torch.float32)
        if return_trace:
            res["trace_parent"] = new("trace_parent", shp(P, B, N), torch.int32)
            res["trace_token"] = new("trace_token", shp(P, B, N), torch.int32)
            res["trace_score"] = new("trace_score", shp(P, B, N), torch.float64)
        joint = ctc_probs is not None or ctc_weight != 0.0
        if joint:
            cp = None if ctc_probs is None else torch.as_tensor(ctc_probs, dtype=torch.float32).to(dev).contiguous()
            assert cp is None or (cp.dim() == 3 and cp.shape[:2] == (B, Tp)), "ctc_probs is [B, Tp, V] of the same encode"
            if return_token_logp:
                res["token_ctc"] = new("token_ctc", shp(B, N, P + 1), torch.float32)
            if return_trace:
                res["trace_ctc"] = new("trace_ctc", shp(P, B, N), torch.float32)
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(dev):
            if workspace is None:
                need = self.decode_workspace_bytes(B, Tp, N, P, joint=joint)
                key = torch.cuda.current_stream(dev).cuda_stream
                workspace = self._ws.get(key)
                if workspace is None or workspace.numel() < need:
                    workspace = self._ws[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            if joint:
                _lib.check(self.lib.ppasr_attention_decode_joint(
                    self._h, memory.data_ptr(), ptr(ol), B, Tp, N, P, ptr(cp), self.vocab_size if cp is None else cp.shape[2],
                    int(blank), float(ctc_weight), res["tokens"].data_ptr(), res["lens"].data_ptr(), res["scores"].data_ptr(),
                    res["ended"].data_ptr(), res["steps_run"].data_ptr(), ptr(res.get("token_logp")),
                    ptr(res.get("token_ctc")), ptr(res.get("trace_parent")), ptr(res.get("trace_token")),
                    ptr(res.get("trace_score")), ptr(res.get("trace_ctc")), workspace.data_ptr(), workspace.numel(), stream))
                return res
            _lib.check(self.lib.ppasr_attention_decode(
                self._h, memory.data_ptr(), ptr(ol), B, Tp, N, P, res["tokens"].data_ptr(), res["lens"].data_ptr(),
                res["scores"].data_ptr(), res["ended"].data_ptr(), res["steps_run"].data_ptr(), ptr(res.get("token_logp")),
                ptr(res.get("trace_parent")), ptr(res.get("trace_token")), ptr(res.get("trace_score")),
                workspace.data_ptr(), workspace.numel(), stream))
        return res

    def loss(self, memory, out_lens, labels, label_lens, lsm_weight=0.0, reverse_weight=0.0, workspace=None, out=None):
        """The label-smoothing loss of the decoder, teacher-forced over one label per utterance (``ppasr_rescorer_loss``):
        memory [B, Tp, D] f32, out_lens [B] i32 or None, labels [B, max_tokens] i32 (only the first label_lens[b] of a row
        are read), label_lens [B] i32 -> dict of device tensors: att_kl, r_att_kl [B] f64 (the sums of the row KL terms
        over the label_lens[b] + 1 target rows of the left decoder, and of the right decoder over the reversed label; 0
        when ``reverse_weight`` is 0), rows [B] i32.  At ``lsm_weight = 0``, att_kl is ``-att`` of ``rescore`` on the same
        label.  Asynchronous on the current stream.  ``workspace`` / ``out``: caller-owned buffers (tests)."""
        dev = self.device
        memory = torch.as_tensor(memory, dtype=torch.float32).to(dev).contiguous()
        labels = torch.as_tensor(labels, dtype=torch.int32).to(dev).contiguous()
        label_lens = torch.as_tensor(label_lens, dtype=torch.int32).to(dev).contiguous()
        ol = None if out_lens is None else torch.as_tensor(out_lens, dtype=torch.int32).to(dev).contiguous()
        B, Tp, D = memory.shape
        mt = labels.shape[1]
        assert D == self.d_model and labels.shape[0] == B and label_lens.shape == (B,)
        o = {} if out is None else out
        new = lambda name, dt: o[name] if name in o else torch.empty((B,), dtype=dt, device=dev)
        res = dict(att_kl=new("att_kl", torch.float64), r_att_kl=new("r_att_kl", torch.float64), rows=new("rows", torch.int32))
        with torch.cuda.device(dev):
            if workspace is None:
                need = int(self.lib.ppasr_rescorer_loss_workspace_bytes(self._h, B, Tp, mt))
                key = torch.cuda.current_stream(dev).cuda_stream
                workspace = self._ws.get(key)
                if workspace is None or workspace.numel() < need:
                    workspace = self._ws[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(self.lib.ppasr_rescorer_loss(self._h, memory.data_ptr(), None if ol is None else ol.data_ptr(), B, Tp,
                                                    labels.data_ptr() if mt else None, label_lens.data_ptr(), mt,
                                                    float(lsm_weight), float(reverse_weight), res["att_kl"].data_ptr(),
                                                    res["r_att_kl"].data_ptr(), res["rows"].data_ptr(),
                                                    workspace.data_ptr(), workspace.numel(), stream))
        return res


def attention_rescoring(model, rescorer, probs, memory, out_lens, vocabulary, beam_size=10, ctc_weight=0.5,
                        reverse_weight=0.0, cutoff_prob=0.99, cutoff_top_n=40, blank_id=0, return_ids=False):
    """probs [B, T', V] and memory [B, T', D] of one encode (``model.get_encoder_out(..., return_memory=True)``),
    out_lens [B] valid frames or None -> per utterance ``(score, text)`` of the hypothesis with the largest total score.
    The n-best list is the plain CTC prefix beam search's (no external scorer); search and rescoring are queued on the
    current stream and read back once.  ``return_ids``: ``(score, text, ids)``, the token ids the text was made of (for
    ``ctc_alignment``)."""
    del model  # (kept in the signature for symmetry with the other decoders: the encode already happened)
    fl = None if out_lens is None else torch.as_tensor(out_lens, dtype=torch.int32)
    tokens, lens, scores, _ = beam_search_ids(probs, beam_size, cutoff_prob, cutoff_top_n, blank_id, frame_lens=fl,
                                              nbest=beam_size)
    if tokens.shape[2] > MAX_ROWS - 1:  # the kernels take 255 tokens per hypothesis; longer ones are refused below
        tokens = tokens[:, :, :MAX_ROWS - 1].contiguous()
    res = rescorer.rescore(memory, fl, tokens, lens, scores, ctc_weight, reverse_weight)
    best = res["best"].to(torch.int64)
    idx = best[:, None, None].expand(-1, 1, tokens.shape[2])
    pack = (tokens.gather(1, idx)[:, 0], lens.gather(1, best[:, None])[:, 0], res["total"].gather(1, best[:, None])[:, 0],
            lens.max())
    tk, ln, sc, longest = [t.cpu().numpy() for t in pack]  # (the read-back)
    if int(longest) > tokens.shape[2]:
        raise _lib.PPASRHipError(f"attention rescoring: a hypothesis of {int(longest)} tokens exceeds the "
                                 f"{MAX_ROWS - 1} the kernels are built for; decode shorter segments",
                                 _lib.PPASR_EUNSUPPORTED)
    ids = [tk[b, :max(int(ln[b]), 0)].tolist() for b in range(tk.shape[0])]
    return [(float(sc[b]), _text(ids[b], vocabulary)) + ((ids[b],) if return_ids else ()) for b in range(tk.shape[0])]
