"""Batched evaluation harness: ``PPASRTrainer.evaluate`` (ppasr/trainer.py:592-645) and ``__decoder_result`` (:330-352)
on top of the HIP hot path.  ``evaluate`` returns the mean CER / WER; with ``return_loss=True`` it returns the
reference's pair ``(loss, error_rate)``, the loss being ``model.forward``'s (CTC and attention losses, forward only:
``model_utils/loss``).  Training itself (backward pass, dropout) is not built.

With ``torch.distributed`` initialised, every rank evaluates the batches ``rank::world`` and the per-utterance error
rates are summed with one all-reduce (utterance data parallelism, NOTES.md §6).  For variable-length batches
``shard="buckets"`` splits EVERY batch over the ranks instead (``parallel.decode_ragged``: whole length buckets per rank
by padded work, one all-gather of the hypotheses per batch), so that ranks finish together whatever the batch order."""
import torch

from ppasr_amd.decoders.beam_search_decoder import beam_search_ids
from ppasr_amd.decoders.ctc_greedy_decoder import greedy_decode_ids, greedy_decoder_batch
from ppasr_amd.parallel import set_skip_padding_if_built
from ppasr_amd.utils.metrics import cer, labels_to_string, wer

__all__ = ["decoder_result", "evaluate"]


def _ids_to_text(ids, vocabulary, greedy):
    """Token ids -> string the way the reference's two decoders do it: greedy_decoder replaces "<space>" by " "
    (ctc_greedy_decoder.py:31); the beam-search module joins the vocabulary entries as they are (its vocabulary is handed
    over with " " already in place, beam_search_decoder.py:59-73)."""
    text = "".join(vocabulary[i] for i in ids)
    return text.replace("<space>", " ") if greedy else text


def _use_greedy(decoder, beam_search_decoder):
    return decoder == "ctc_greedy" or beam_search_decoder is None


def _reset_scorer(beam_search_decoder):
    """decode_batch_beam_search_offline re-applies the decoder object's alpha / beta to the scorer on every call
    (beam_search_decoder.py:60-61); every beam route of this module does the same, so alpha / beta tuned on the decoder
    object after construction are honoured whichever route decodes."""
    sc = getattr(beam_search_decoder, "_ext_scorer", None)
    if sc is not None:
        sc.reset_params(beam_search_decoder.alpha, beam_search_decoder.beta)


def decoder_result(outs, vocabulary, decoder="ctc_greedy", beam_search_decoder=None, frame_lens=None):
    """trainer.py:330-352: outs [B,T',V] (device tensor or numpy) -> list[str]; every one of the T' rows is decoded
    (the reference's behaviour) unless ``frame_lens`` [B] names the valid frames of every utterance."""
    if frame_lens is None:
        if decoder == "ctc_greedy" or beam_search_decoder is None:
            return greedy_decoder_batch(outs, vocabulary)
        return beam_search_decoder.decode_batch_beam_search_offline(probs_split=outs)
    greedy = _use_greedy(decoder, beam_search_decoder)
    if greedy:
        tokens, n, _, _, _ = greedy_decode_ids(outs, frame_lens)
    else:
        d = beam_search_decoder
        _reset_scorer(d)
        tokens, n, _, _ = beam_search_ids(outs, d.beam_size, d.cutoff_prob, d.cutoff_top_n, d.blank_id,
                                          frame_lens=frame_lens, nbest=1, ext_scorer=d._ext_scorer)
        tokens, n = tokens[:, 0], n[:, 0]
    tk, nn = tokens.cpu(), n.cpu()
    return [_ids_to_text(tk[b, :max(int(nn[b]), 0)].tolist(), vocabulary, greedy) for b in range(tk.shape[0])]


def evaluate(model, batches, vocab_list, decoder="ctc_greedy", metrics_type="cer", beam_search_decoder=None,
             display_result=False, trim_padding=False, overlap_decode=True, shard="batches", rescorer=None,
             rescoring_conf=None, return_loss=False, loss_conf=None, attention_conf=None):
    """model: any ppasr_amd model with ``get_encoder_out(inputs, input_lens)``;
    batches: iterable of (inputs [B,T,F], labels [B,U] (-1 padded), input_lens [B], label_lens [B]) like the reference's
    test_loader.  -> mean error rate (float), -1 if there is nothing to score (trainer.py:643).
    ``trim_padding=True`` (not the reference's behaviour, which decodes the padded rows of every utterance too): the
    encoder runs in its ragged-batch mode and the decoders stop at each utterance's last valid frame.
    ``overlap_decode``: encode batch i+1 on a second HIP stream while batch i is being decoded (same results).
    ``shard``: "batches" = batch i goes to rank i % world; "buckets" = every batch is cut into length buckets that are
    dealt to the ranks by padded work (ragged batches).  "buckets" ALWAYS has ``trim_padding=True`` semantics -- the
    encoder skips the padding and decoding covers each utterance's valid frames only, whatever ``trim_padding`` says --
    so for batches with padding its error rate equals ``shard="batches", trim_padding=True``, not the reference's
    padded-row decoding; with ``decoder != "ctc_greedy"`` a ``beam_search_decoder`` is required (no silent greedy).
    ``decoder="attention_rescoring"``: ``rescorer`` (an ``AttentionRescorer`` of the same checkpoint) is required and
    ``rescoring_conf`` holds the keyword arguments of ``decoders.attention_rescoring.attention_rescoring`` (beam_size,
    ctc_weight, reverse_weight, cutoff_prob, cutoff_top_n); ``shard="batches"`` only, encode and decode on one stream.
    ``decoder="attention"``: the attention beam search (``decoders.attention_decoder.attention_decode``); ``rescorer`` is
    required likewise and ``attention_conf`` holds ``beam_size``, ``max_steps`` and ``ctc_weight`` (above 0: CTC-joint scoring
    inside the search, on the table of the same encode); ``shard="batches"`` only, one stream.
    ``return_loss=True``: -> ``(loss, error_rate)`` like the reference; ``loss`` is the mean over batches of
    ``model_loss(...)["loss"] / accum_grad`` (trainer.py:624, 642; -1 without batches) with ``loss_conf`` holding
    ``ctc_weight`` (default 0.5; a DeepSpeech2 model's loss is its CTC loss alone), ``lsm_weight``, ``reverse_weight``,
    ``length_normalized_loss`` and ``accum_grad``.  ``ctc_weight < 1`` needs ``rescorer``; ``shard="batches"`` only, encode
    and decode on one stream.  The error rate is the one the same call returns without ``return_loss``."""
    attention = decoder == "attention"
    rescoring = decoder == "attention_rescoring" or attention  # (what follows: the decode reads the encoder output)
    if rescoring and (rescorer is None or shard != "batches"):
        raise ValueError(f"decoder={decoder!r} needs a rescorer and shard='batches'")
    if return_loss:
        from ppasr_amd.model_utils.loss import _branches, encode_for_loss, loss_of_encoded
        if shard != "batches":
            raise ValueError("return_loss=True needs shard='batches'")
        lc = dict(loss_conf or {})
        accum_grad = float(lc.pop("accum_grad", 1))
        loss_kw = dict(lsm_weight=float(lc.pop("lsm_weight", 0.0)), reverse_weight=float(lc.pop("reverse_weight", 0.0)),
                       length_normalized_loss=bool(lc.pop("length_normalized_loss", False)))
        loss_cw = _branches(model, rescorer, lc.pop("ctc_weight", 0.5))
        if lc:
            raise ValueError("unknown loss_conf keys: " + ", ".join(sorted(lc)))
        want_memory = loss_cw != 1.0
    else:
        want_memory = False
    loss_total, loss_batches = 0.0, 0
    dist = torch.distributed.is_available() and torch.distributed.is_initialized()
    if shard == "buckets":
        return _evaluate_bucketed(model, batches, vocab_list, decoder, metrics_type, beam_search_decoder, display_result,
                                  torch.distributed if dist else None)
    if shard != "batches":
        raise ValueError(f"shard={shard!r}: 'batches' or 'buckets'")
    rank = torch.distributed.get_rank() if dist else 0
    world = torch.distributed.get_world_size() if dist else 1
    eos = len(vocab_list) - 1
    total, count = 0.0, 0
    dev = getattr(model, "device", None)
    pipelined = overlap_decode and dev is not None and torch.device(dev).type == "cuda" and not rescoring and not return_loss
    enc_stream = torch.cuda.Stream(device=dev) if pipelined else None

    def encode(inputs, input_lens):
        frame_lens = None
        if trim_padding:
            set_skip_padding_if_built(model, True)
            frame_lens = model.valid_out_frames(input_lens, inputs.shape[1])
        try:
            outs = model.get_encoder_out(inputs, input_lens, return_memory=True) if rescoring or want_memory else \
                model.get_encoder_out(inputs, input_lens)
        finally:
            if trim_padding:
                set_skip_padding_if_built(model, False)
        return outs, frame_lens

    def score(outs, frame_lens, labels):
        nonlocal total, count
        if attention:
            from ppasr_amd.decoders.attention_decoder import attention_decode
            out_strings = [t for _, t in attention_decode(model, rescorer, outs[1], frame_lens, vocab_list, probs=outs[0],
                                                          **dict(attention_conf or {}))]
        elif rescoring:
            from ppasr_amd.decoders.attention_rescoring import attention_rescoring
            out_strings = [t for _, t in attention_rescoring(model, rescorer, outs[0], outs[1], frame_lens, vocab_list,
                                                             **dict(rescoring_conf or {}))]
        else:
            out_strings = decoder_result(outs, vocab_list, decoder, beam_search_decoder, frame_lens)
        labels_str = labels_to_string(labels, vocab_list, eos=eos)
        for out_string, label in zip(out_strings, labels_str):
            err = wer(out_string, label) if metrics_type == "wer" else cer(out_string, label)
            total += err
            count += 1
            if display_result:
                print(f"pred: {out_string}\nlabel: {label}\n{metrics_type}: {round(err, 6)}")

    # Two-stage pipeline on two HIP streams: the encoder of batch i+1 is queued on its own stream before the host waits
    # for the decode of batch i (beam search occupies one CU per utterance -- the rest of the chip encodes meanwhile).
    pending = None  # (outs, frame_lens, labels, event) of the batch whose decode has not run yet
    for batch_id, (inputs, labels, input_lens, _label_lens) in enumerate(batches):
        if batch_id % world != rank:
            continue
        if not pipelined:
            if return_loss and not hasattr(model, "valid_out_frames"):  # DeepSpeech2: the encode itself returns the frames
                probs, memory, frames = encode_for_loss(model, inputs, input_lens, False)
                outs, frame_lens = probs, None
            else:
                outs, frame_lens = encode(inputs, input_lens)
            if return_loss:  # the loss reads the probabilities (and the encoder output) the decode below reads
                if hasattr(model, "valid_out_frames"):
                    probs, memory = outs if rescoring or want_memory else (outs, None)
                    frames = model.valid_out_frames(input_lens, inputs.shape[1])
                loss_total += loss_of_encoded(rescorer, probs, memory, frames, labels, _label_lens, loss_cw,
                                              **loss_kw)["loss"] / accum_grad
                loss_batches += 1
                if not rescoring:
                    outs = probs
            score(outs, frame_lens, labels)
            continue
        dec_stream = torch.cuda.current_stream(dev)
        enc_stream.wait_stream(dec_stream)  # (inputs prepared on the caller's stream)
        with torch.cuda.stream(enc_stream):
            outs, frame_lens = encode(inputs, input_lens)
            ev = torch.cuda.Event()
            ev.record(enc_stream)
        if pending is not None:
            score(*pending[:3])
        dec_stream.wait_event(ev)
        outs.record_stream(dec_stream)
        if frame_lens is not None:
            frame_lens.record_stream(dec_stream)
        pending = (outs, frame_lens, labels)
    if pending is not None:
        score(*pending[:3])
    if dist:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.distributed.get_backend() == "nccl" else "cpu"
        t = torch.tensor([total, float(count), loss_total, float(loss_batches)], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t)
        total, count, loss_total, loss_batches = float(t[0]), int(t[1]), float(t[2]), int(t[3])
    if return_loss:
        return (loss_total / loss_batches if loss_batches > 0 else -1), (total / count if count > 0 else -1)
    return total / count if count > 0 else -1


def _evaluate_bucketed(model, batches, vocab_list, decoder, metrics_type, beam_search_decoder, display_result, dist):
    """Every rank walks every batch and decodes ITS length buckets of it; after the gather each rank holds all
    hypotheses of the batch, so the error sums are identical on every rank and need no further collective."""
    from ppasr_amd.parallel import beam_ids_decoder, decode_ragged, greedy_ids_decoder
    if decoder != "ctc_greedy" and beam_search_decoder is None:
        raise ValueError(f"evaluate(shard='buckets', decoder={decoder!r}) needs a beam_search_decoder")
    greedy = _use_greedy(decoder, beam_search_decoder)
    if greedy:
        dec = greedy_ids_decoder()
    else:
        d = beam_search_decoder
        _reset_scorer(d)
        dec = beam_ids_decoder(d.beam_size, d.cutoff_prob, d.cutoff_top_n, d.blank_id, d._ext_scorer)
    eos = len(vocab_list) - 1
    total, count = 0.0, 0
    for inputs, labels, input_lens, _label_lens in batches:
        lens = [int(v) for v in torch.as_tensor(input_lens).tolist()]
        tokens, n, _ = decode_ragged(model, inputs, lens, dec, dist=dist)
        tk, nn = tokens.cpu(), n.cpu()
        labels_str = labels_to_string(labels, vocab_list, eos=eos)
        for b, label in enumerate(labels_str):
            out_string = _ids_to_text(tk[b, :max(int(nn[b]), 0)].tolist(), vocab_list, greedy)
            err = wer(out_string, label) if metrics_type == "wer" else cer(out_string, label)
            total += err
            count += 1
            if display_result:
                print(f"pred: {out_string}\nlabel: {label}\n{metrics_type}: {round(err, 6)}")
    return total / count if count > 0 else -1
