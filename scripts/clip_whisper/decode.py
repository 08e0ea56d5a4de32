#!/usr/bin/env python3
"""Decode -> WER entry point.  Takes the reference's command line as given (scripts/clip_whisper/decode.py:42-66:
--model_path --test_data --test_wrd --output_dir --modality --batch_size --max_new_tokens --temperature --device --seed --config
--verbose --whisper_model --clip_model --llm_model --calculate_loss --text_key --output_file) and does what that script does:
rebuild the model WITHOUT adapters, load ONLY the connector tensors from the checkpoint (decode.py:236-260), map utterance ids of the
manifest to the lines of the .wrd file (:318-372, with the path-less id as a second key), greedy `generate` at max_seq_len 256,
`batch_decode`, per-utterance and corpus WER, and the same files: decode_<ts>.log, results_<ts>.txt (the reference's table),
wer_<ts>.txt ("Overall WER" / "Total samples").

Additions of this build (not reference flags): --do_sample / --top_p (default 0.9) / --top_k (default 50) (sampled `generate`:
temperature -> top-k -> top-p on the device, its seed drawn after torch.manual_seed(--seed); without --do_sample decoding stays
greedy and --temperature is ignored, as in the reference), --num_beams (default 1: greedy or sampled as above) / --length_penalty
(default 1.0) (HF beam search, the best hypothesis per utterance), --repetition_penalty (default 1.0) / --no_repeat_ngram_size (default 0) /
--min_new_tokens (default 0) (HF's logits processors of those names, on the device, in every decoding mode), --suppress_tokens /
--begin_suppress_tokens (comma-separated token ids, or @FILE with ids separated by commas or white space: never generated / not generated
as the first token), --bad_words FILE (one phrase per line, never generated: each is tokenised with and without a leading space and
passed as bad_words_ids), --hotwords FILE (one word or phrase per line) / --hotword_bias F (added to the score of every token on the
path of a hotword; generate(hotwords=, hotword_bias=)), --nbest N (beam search returns the N best hypotheses of each utterance; needs
--num_beams >= N; WER stays on the 1-best), --confidence (adds tokens, token_logprobs, avg_logprob and word_confidences of the 1-best to each
utterance of the --output_file JSON, and with --nbest > 1 an nbest list of {hypothesis, score}), --min_avg_logprob F (utterances whose mean
token log-probability is below F are listed in the log; they still count in the WER), --share_prefix (generate(share_prefix=True): the beams
of an utterance share one prefix cache), --load_lora (also load the adapters from the checkpoint), --lora_target_modules (with --load_lora: the modules those adapters sit on,
default what the checkpoint's metadata records; adapters on gate/up/down keep the token step off the fused path until --merge_lora folds them),--merge_lora (with --load_lora: fold the loaded
adapters into the LLM weights once, ClipWhisperModel.merge_lora(), so that decoding runs the adapter-free kernels), --drop_audio_prob F /
--drop_video_prob F (robustness evaluation with --modality both: every clip loses its audio / its video with that probability, never both;
the modes of batch k are drawn on the device with seed --seed + k, so a run repeats, and go to generate(modality_mask=); the results JSON
records the two probabilities and the number of clips per mode), --noise_path P --noise_snr F [--noise_prob F] (robustness evaluation at
a fixed SNR: a segment of a noise recording under P is mixed into each clip's waveform on the device before the log-mel, batch k drawn with
seed --seed + k, so a sweep over --noise_snr mixes the same segments and only their level changes; needs a manifest dataset, whose audio is
raw; the results JSON records the path, the SNR and the number of clips mixed), --synthetic N / --tiny /
--synthetic-weights / --frames (no dataset or checkpoints offline), --data_path (root for relative media paths; default = the
reference's rule dirname(dirname(test_data))), and --test_manifest / --test_labels as aliases of --test_data / --test_wrd.
`--output_file` (declared but never written by the reference) receives the per-utterance results as JSON."""
import argparse
import json
import logging
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "audio-visual-llm_amd")):
    sys.path.insert(0, p) if p not in sys.path else None

import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Run inference with the ClipWhisperModel and calculate WER")
    p.add_argument("--model_path", type=str, help="Path to the trained checkpoint (.pt)")
    p.add_argument("--test_data", "--test_manifest", dest="test_data", type=str, help="Path to test data TSV file")
    p.add_argument("--test_wrd", "--test_labels", dest="test_wrd", type=str, help="Path to test word reference file")
    p.add_argument("--output_dir", type=str, default="outputs/clip_whisper_decoding")
    p.add_argument("--modality", type=str, choices=["audio", "video", "both"], default="both")
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--max_new_tokens", type=int, default=100)
    p.add_argument("--temperature", type=float, default=1.0)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--config", type=str, default=os.path.join(ROOT, "configs", "clip_whisper.yaml"))
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--whisper_model", type=str, default=None, help="overrides the YAML's whisper_model")
    p.add_argument("--clip_model", type=str, default=None, help="overrides the YAML's clip_model")
    p.add_argument("--llm_model", type=str, default=None, help="overrides the YAML's llm_path")
    p.add_argument("--calculate_loss", action="store_true", help="also report the eval loss against the reference text")
    p.add_argument("--text_key", type=str, default="text")
    p.add_argument("--output_file", type=str, default="decode_results.json")
    # ---- this build's additions
    p.add_argument("--do_sample", action="store_true", help="sample instead of greedy decoding (temperature, top_k, top_p)")
    p.add_argument("--top_p", type=float, default=0.9)
    p.add_argument("--top_k", type=int, default=50, help="0 turns top-k off")
    p.add_argument("--num_beams", type=int, default=1, help="beam search with this many beams (1 = greedy / sampling)")
    p.add_argument("--length_penalty", type=float, default=1.0, help="beam search: scores are divided by length ** length_penalty")
    p.add_argument("--repetition_penalty", type=float, default=1.0, help="> 1 lowers the score of every token already generated (1.0 = off)")
    p.add_argument("--no_repeat_ngram_size", type=int, default=0, help="no n-gram of this size is generated twice (0 = off)")
    p.add_argument("--min_new_tokens", type=int, default=0, help="EOS is not generated before this many new tokens")
    p.add_argument("--suppress_tokens", type=str, default=None, help="token ids that are never generated: 1,2,3 or @FILE")
    p.add_argument("--begin_suppress_tokens", type=str, default=None, help="token ids not generated as the first token: 1,2,3 or @FILE")
    p.add_argument("--bad_words", type=str, default=None, help="file with one phrase per line that is never generated")
    p.add_argument("--hotwords", type=str, default=None, help="file with one word or phrase per line to boost (contextual biasing)")
    p.add_argument("--hotword_bias", type=float, default=0.0, help="added to the score of every token on a hotword's path")
    p.add_argument("--nbest", type=int, default=1, help="beam search: the N best hypotheses per utterance (needs --num_beams >= N)")
    p.add_argument("--confidence", action="store_true", help="token log-probabilities and word confidences in the --output_file JSON")
    p.add_argument("--min_avg_logprob", type=float, default=None, help="list utterances whose mean token log-probability is below this")
    p.add_argument("--decode_weights", type=str, choices=["bf16", "fp8", "fp4"], default="bf16",
                   help="fp8: the token steps stream the LLM's frozen projections as block-scaled e4m3 (needs bf16; prefill stays bf16); "
                        "fp4: as OCP MXFP4 with lm_head as e4m3 (coarser: about 11.5 %% weight error, effect on WER not measured)")
    p.add_argument("--kv_cache", type=str, choices=["bf16", "fp8"], default="bf16",
                   help="fp8: the KV cache is block-scaled e4m3 (33/64 of the bf16 bytes; needs bf16, token steps of at most 16 rows, else "
                        "the bf16 cache is used; effect on WER not measured)")
    p.add_argument("--share_prefix", action="store_true",
                   help="generate(share_prefix=True): the beams of an utterance (--num_beams > 1) read one copy of its prefix cache and keep only "
                        "their generated positions (token steps of at most 16 rows, bf16; otherwise the default path is taken).  generate() "
                        "shares the same way among the n sampled sequences of num_return_sequences=n; this script samples one per utterance, "
                        "and greedy decoding has nothing to share")
    p.add_argument("--load_lora", action="store_true")
    p.add_argument("--lora_target_modules", type=str, default=None,
                   help="with --load_lora: the modules the checkpoint's adapters sit on (comma-separated names out of q_proj,k_proj,v_proj,o_proj,"
                        "gate_proj,up_proj,down_proj, or all-linear).  Default: the YAML's model.lora_target_modules, else what the checkpoint's "
                        "_meta.json records, else the four attention modules.  An unmerged adapter on gate/up/down keeps the token step off "
                        "the fused path: add --merge_lora")
    p.add_argument("--merge_lora", action="store_true",
                   help="with --load_lora: fold the adapters into the LLM weights after the checkpoint is loaded (effect on WER not measured)")
    p.add_argument("--drop_audio_prob", type=float, default=0.0,
                   help="robustness evaluation: each clip is decoded without its audio with this probability (needs --modality both)")
    p.add_argument("--drop_video_prob", type=float, default=0.0,
                   help="... or without its video with this one; the two add up to at most 1, a clip never loses both")
    p.add_argument("--noise_path", type=str, default=None,
                   help="robustness evaluation: a .wav / .npy noise recording or a directory of them (16 kHz), mixed into every clip's audio")
    p.add_argument("--noise_snr", type=float, default=None, help="with --noise_path: the SNR in dB of every mixed clip")
    p.add_argument("--noise_prob", type=float, default=1.0, help="with --noise_path: the share of clips that get noise (default all)")
    p.add_argument("--data_path", type=str, default=None)
    p.add_argument("--synthetic", type=int, default=0)
    p.add_argument("--tiny", action="store_true")
    p.add_argument("--frames", type=int, default=125)
    p.add_argument("--synthetic-weights", action="store_true", help="seeded random weights + byte tokenizer (implied by --tiny)")
    a = p.parse_args(argv)
    if a.lora_target_modules and not a.load_lora:
        p.error("--lora_target_modules needs --load_lora: without it the model has no adapters")
    if a.merge_lora and not a.load_lora:
        p.error("--merge_lora needs --load_lora: without it the model has no adapters to merge")
    if not (0.0 <= a.drop_audio_prob <= 1.0 and 0.0 <= a.drop_video_prob <= 1.0 and a.drop_audio_prob + a.drop_video_prob <= 1.0):
        p.error(f"--drop_audio_prob {a.drop_audio_prob} and --drop_video_prob {a.drop_video_prob} must lie in [0, 1] and add up to at most 1")
    if (a.drop_audio_prob or a.drop_video_prob) and a.modality != "both":
        p.error(f"--drop_audio_prob / --drop_video_prob need --modality both, got --modality {a.modality}")
    if (a.noise_path is None) != (a.noise_snr is None):
        p.error("--noise_path and --noise_snr go together: the recordings and the SNR in dB at which they are mixed in")
    if a.noise_path is not None and a.synthetic:
        p.error("--noise_path needs raw audio (a manifest dataset): --synthetic clips are precomputed features")
    if a.noise_path is not None and a.modality == "video":
        p.error("--noise_path needs the audio stream, got --modality video")
    if not 0.0 <= a.noise_prob <= 1.0:
        p.error(f"--noise_prob {a.noise_prob} must lie in [0, 1]")
    if a.nbest < 1:
        p.error(f"--nbest must be at least 1, got {a.nbest}")
    if a.nbest > 1 and a.do_sample:
        p.error("--nbest > 1 is beam search: it cannot be combined with --do_sample")
    if a.nbest > 1 and a.num_beams < a.nbest:
        p.error(f"--nbest {a.nbest} needs --num_beams >= {a.nbest}, got --num_beams {a.num_beams}")
    return a


def token_id_list(arg):
    """--suppress_tokens / --begin_suppress_tokens: '1,2,3', or '@FILE' holding ids separated by commas or white space."""
    if arg is None:
        return None
    text = open(arg[1:]).read() if arg.startswith("@") else arg
    return [int(t) for t in text.replace(",", " ").split()]


def lines_of(path):
    return None if path is None else [ln.strip() for ln in open(path) if ln.strip()]


def match_references(ids, texts):
    """utterance id -> reference text, ids and .wrd lines paired by position (decode.py:318-372); the last path component of an id is a
    second key.  `ids` are the manifest's well-formed entries (the dataset's own list, so ids and samples cannot drift apart: the
    reference script re-parses the TSV with a looser rule than its dataset and shifts every reference by one on a malformed line)."""
    if len(ids) != len(texts):
        logging.warning(f"Mismatch between number of utterance IDs ({len(ids)}) and reference texts ({len(texts)})")
    refs = {}
    for uid, t in zip(ids, texts):
        refs[uid] = t
        if "/" in uid:
            refs[uid.split("/")[-1]] = t
    return refs


def utterance_scores(tokenizer, out, nbest, eos):
    """--confidence: per utterance, from generate(return_token_scores=True, num_return_sequences=nbest): the 1-best's tokens (up to and
    including its EOS), their log-probabilities, the mean of those, its word confidences, and with nbest > 1 the n-best list."""
    from avllm.confidence import word_confidences
    seqs, lps = out.sequences.cpu(), out.token_scores.cpu()
    scores = None if out.sequences_scores is None else out.sequences_scores.cpu().tolist()
    conf = word_confidences(tokenizer, seqs[::nbest], lps[::nbest])
    res = []
    for u in range(seqs.shape[0] // nbest):
        row = seqs[u * nbest].tolist()
        n = row.index(eos) + 1 if eos is not None and eos in row else len(row)
        tl = [float(v) for v in lps[u * nbest, :n]]
        d = {"tokens": row[:n], "token_logprobs": tl, "avg_logprob": sum(tl) / max(len(tl), 1),
             "word_confidences": [[w, c] for w, c in conf[u]]}
        if nbest > 1:
            hyps = tokenizer.batch_decode(seqs[u * nbest:(u + 1) * nbest], skip_special_tokens=True)
            d["nbest"] = [{"hypothesis": h.strip(), "score": scores[u * nbest + i]} for i, h in enumerate(hyps)]
        res.append(d)
    return res


def main(argv=None):
    a = parse_args(argv)
    torch.manual_seed(a.seed)
    os.makedirs(a.output_dir, exist_ok=True)
    ts = time.strftime("%Y%m%d_%H%M%S")
    root_logger = logging.getLogger()
    for h in root_logger.handlers[:]:
        root_logger.removeHandler(h)
    fh = logging.FileHandler(os.path.join(a.output_dir, f"decode_{ts}.log"))
    fh.setLevel(logging.DEBUG if a.verbose else logging.INFO)
    ch = logging.StreamHandler()
    ch.setLevel(logging.WARNING)
    root_logger.setLevel(logging.DEBUG if a.verbose else logging.INFO)
    root_logger.addHandler(fh); root_logger.addHandler(ch)
    logging.info(f"Model path: {a.model_path}  Modality: {a.modality}  Test data: {a.test_data}  Test references: {a.test_wrd}  Device: {a.device}")
    print("\n" + "=" * 80 + f"\nCLIP-WHISPER DECODING\nModel: {a.model_path}\nModality: {a.modality}\n" + "=" * 80 + "\n")

    from avllm.config import merged
    from avllm.model import ClipWhisperModel
    from avllm.wer import calculate_wer
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from train import SyntheticClips
    cfg = merged(a.config, {"llm_path": a.llm_model, "whisper_model": a.whisper_model, "clip_model": a.clip_model})
    dev = "cuda:0" if a.device in ("cuda", "gpu") else a.device
    if not dev.startswith("cuda"):
        raise ValueError(f"--device {a.device}: this build runs the path on an MI355X only (there is no CPU fallback)")
    kw = {}
    if a.load_lora:
        targets = a.lora_target_modules or cfg.get("lora_target_modules")
        if targets is None and a.model_path:
            from avllm.trainer import ClipWhisperTrainer
            targets = ClipWhisperTrainer.checkpoint_lora_targets(a.model_path)
        if targets is not None:
            kw["lora_target_modules"] = targets
    if a.tiny:
        from avllm.arch import ClipCfg, LlamaCfg, LoraCfg, ModelCfg, WhisperCfg
        kw["config"] = ModelCfg(WhisperCfg(128, 2, 2, 256), ClipCfg(128, 2, 2, 256, 48, 16), LlamaCfg(256, 2, 2, 512, 512), LoraCfg(16, 32.0))
    model = ClipWhisperModel(llm_path=cfg["llm_path"], whisper_model=cfg["whisper_model"], clip_model=cfg["clip_model"], device=dev,
                             use_fp16=bool(cfg.get("use_fp16")), use_lora=a.load_lora, modality=a.modality, max_seq_len=256,
                             synthetic_weights=a.synthetic_weights or a.tiny, decode_weights=a.decode_weights, kv_cache=a.kv_cache, **kw).eval()
    if a.model_path:
        ck = torch.load(a.model_path, map_location="cpu", weights_only=True)
        sd = ck.get("model_state_dict", ck)
        keep = {k: v for k, v in sd.items() if "audio_connector" in k or "video_connector" in k or (a.load_lora and "lora_" in k)}
        if not any("audio_connector" in k for k in keep):
            logging.warning("No audio connector weights found in checkpoint")
        if not any("video_connector" in k for k in keep):
            logging.warning("No video connector weights found in checkpoint")
        model.load_state_dict(keep)
        mc = ck.get("config") if isinstance(ck, dict) else None
        if isinstance(mc, dict):
            model.max_seq_len = mc.get("max_seq_len", 256); model.fusion_scale = mc.get("fusion_scale", 0.5)
    if a.merge_lora:
        model.merge_lora()
        logging.info("LoRA adapters merged into the LLM weights")

    from avllm.tokenizer import phrase_token_ids
    bad_words = lines_of(a.bad_words)
    bias_kw = dict(suppress_tokens=token_id_list(a.suppress_tokens), begin_suppress_tokens=token_id_list(a.begin_suppress_tokens),
                   bad_words_ids=[list(ids) for w in bad_words or [] for ids in phrase_token_ids(model.tokenizer, w)] or None,
                   hotwords=lines_of(a.hotwords), hotword_bias=a.hotword_bias)

    references, utt_ids = {}, None
    noise_mixed = 0                                               # clips that had noise mixed in (--noise_path)
    if a.synthetic:
        ds = SyntheticClips(a.synthetic, model.cfg, 5 if a.tiny else a.frames, model.tokenizer, 11)
        loader = torch.utils.data.DataLoader(ds, batch_size=a.batch_size, collate_fn=ds.collate)
        utt_ids = [f"synthetic_{i}" for i in range(len(ds))]
        references = {utt_ids[i]: ds[i][2] for i in range(len(ds))}

        def batches():
            for b in loader:
                yield b[0], b[1], b[2]
    else:
        droot = a.data_path or cfg.get("path") or "."
        test_data = a.test_data or os.path.join(droot, cfg.get("test_manifest", "test.tsv"))
        test_wrd = a.test_wrd or os.path.join(droot, cfg.get("test_labels", "test.wrd"))
        if not os.path.exists(test_data) or not os.path.exists(test_wrd):
            print("ERROR: Both --test_data and --test_wrd are required for batch decoding mode")
            logging.error("Both --test_data and --test_wrd are required for batch decoding mode")
            return 1
        from avllm.data import AVSRDataset
        from avllm.preprocess import ClipFrames, WhisperLogMel, device_collate
        root = a.data_path or os.path.dirname(os.path.dirname(os.path.abspath(test_data)))       # decode.py:394
        ds = AVSRDataset(test_data, test_wrd, root, model.tokenizer, max_audio_length=30, max_video_length=300, split="test", modality=a.modality)
        utt_ids = [n[2] for n in ds.names]
        references = match_references(utt_ids, ds.labels)
        loader = torch.utils.data.DataLoader(ds, batch_size=a.batch_size, shuffle=False, collate_fn=AVSRDataset.collate_fn)
        feats = (WhisperLogMel(dev, n_mels=model.cfg.whisper.n_mels), ClipFrames(dev, image=model.cfg.clip.image))
        augment = None
        if a.noise_path is not None:
            from avllm.preprocess import AudioAugment, NoiseBank
            augment = AudioAugment(noise=NoiseBank(a.noise_path, dev), snr_db=a.noise_snr, noise_prob=a.noise_prob)

        def batches():
            nonlocal noise_mixed
            for k, b in enumerate(loader):
                if augment is None:
                    audio, video = device_collate(b["raw"], *feats)
                else:
                    audio, video = device_collate(b["raw"], *feats, augment=augment, seed=a.seed + k)
                    if audio is not None:
                        noise_mixed += int(augment.last_info[:, 0].sum())
                yield audio, video, b["texts"]

    scored = a.confidence or a.nbest > 1 or a.min_avg_logprob is not None
    score_kw = dict(return_token_scores=True, num_return_sequences=a.nbest) if scored else {}
    low_confidence = []
    drop = bool(a.drop_audio_prob or a.drop_video_prob)
    mode_counts = [0, 0, 0]                                       # clips decoded with both streams / audio only / video only
    results, all_refs, all_hyps, losses = [], [], [], []
    seen = 0
    print(f"Starting decoding with modality: {a.modality}\nEach hypothesis will be shown as it's generated.\n")
    for bi, (audio, video, texts) in enumerate(batches()):
        try:
            audio = None if (audio is None or a.modality == "video") else audio.to(dev)
            video = None if (video is None or a.modality == "audio") else video.to(dev)
            mask_kw = {}
            if drop:
                from avllm import ops
                modes = ops.modality_draw(audio.shape[0], a.drop_audio_prob, a.drop_video_prob, seed=a.seed + bi, device=dev)
                mask_kw["modality_mask"] = modes
            ids = model.generate(audio=audio, video=video, max_new_tokens=a.max_new_tokens, temperature=a.temperature,
                                 do_sample=a.do_sample, top_p=a.top_p, top_k=a.top_k, num_beams=a.num_beams,
                                 length_penalty=a.length_penalty, repetition_penalty=a.repetition_penalty,
                                 no_repeat_ngram_size=a.no_repeat_ngram_size, min_new_tokens=a.min_new_tokens, share_prefix=a.share_prefix,
                                 **bias_kw, **score_kw, **mask_kw)
            if drop:
                for m in modes.tolist():
                    mode_counts[m] += 1
            extras = None
            if scored:
                extras = utterance_scores(model.tokenizer, ids, a.nbest, model.eos_token_id)
                ids = ids.sequences[::a.nbest]
            out = model.tokenizer.batch_decode(ids.cpu(), skip_special_tokens=True)
            if a.calculate_loss:
                lab = model.tokenizer(list(texts), padding="max_length", truncation=True, max_length=256, return_tensors="pt").input_ids
                with torch.no_grad():
                    losses.append(float(model(audio=audio, video=video, labels=lab.to(dev), return_loss=True, **mask_kw)["loss"]))
            for j, hyp in enumerate(out):
                uid = utt_ids[seen + j] if seen + j < len(utt_ids) else f"unknown_{bi}_{j}"
                hyp = hyp.strip()
                ref = references.get(uid, references.get(uid.split("/")[-1]) if "/" in uid else None)
                print(f"\nUTT: {uid}\nHYP: {hyp}\nREF: {ref if ref is not None else '[None]'}\n" + "-" * 40)
                if ref is not None:
                    all_refs.append(ref); all_hyps.append(hyp)
                    results.append({"utt_id": uid, "hypothesis": hyp, "reference": ref, "wer": calculate_wer([ref], [hyp])})
                    if a.confidence:
                        results[-1].update(extras[j])
                if extras is not None and a.min_avg_logprob is not None and extras[j]["avg_logprob"] < a.min_avg_logprob:
                    low_confidence.append((uid, extras[j]["avg_logprob"]))
            seen += len(out)
        except Exception as e:                                   # noqa: BLE001  decode.py:647-650: log and go on with the next batch
            logging.error(f"Error processing batch {bi}: {e}")
            seen += len(texts)
            continue
    if not all_refs:
        logging.warning("No samples were successfully processed for WER calculation")
        print("\nNo samples were successfully processed for WER calculation")
        return 1
    wer = calculate_wer(all_refs, all_hyps)
    with open(os.path.join(a.output_dir, f"results_{ts}.txt"), "w") as f:
        f.write(f"Modality: {a.modality}\nOverall WER: {wer:.4f}\n\nDetailed Results:\n")
        f.write(f"{'Utterance ID':<20} {'WER':<10} {'Reference':<40} {'Hypothesis':<40}\n" + "-" * 110 + "\n")
        for r in results:
            f.write(f"{r['utt_id']:<20} {r['wer']:<10.4f} {r['reference'][:40]:<40} {r['hypothesis'][:40]:<40}\n")
    with open(os.path.join(a.output_dir, f"wer_{ts}.txt"), "w") as f:
        f.write(f"Overall WER: {wer:.4f}\nTotal samples: {len(all_refs)}\n")
    summary = {"modality": a.modality, "overall_wer": wer, "total_samples": len(all_refs), "results": results}
    if drop:
        summary.update({"drop_audio_prob": a.drop_audio_prob, "drop_video_prob": a.drop_video_prob,
                        "clips_per_mode": {"both": mode_counts[0], "audio": mode_counts[1], "video": mode_counts[2]}})
    if a.noise_path is not None:
        summary.update({"noise_path": a.noise_path, "noise_snr": a.noise_snr, "noise_prob": a.noise_prob, "clips_with_noise": noise_mixed})
    if losses:
        summary["mean_loss"] = sum(losses) / len(losses)
    json.dump(summary, open(os.path.join(a.output_dir, os.path.basename(a.output_file)), "w"), indent=1)
    if a.min_avg_logprob is not None:
        logging.info(f"{len(low_confidence)} utterances with avg_logprob < {a.min_avg_logprob} (kept in the WER):")
        for uid, v in low_confidence:
            logging.info(f"  low confidence: {uid} avg_logprob {v:.4f}")
    logging.info(f"Overall WER: {wer:.4f}")
    print("\n" + "=" * 80 + f"\nDECODING SUMMARY\nModality: {a.modality}\nOverall WER: {wer:.4f}\nTotal samples: {len(all_refs)}\n" + "=" * 80)
    return 0


if __name__ == "__main__":
    sys.exit(main())
