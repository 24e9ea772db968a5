"""TTSEngine -- same class surface as the reference engine (vietvoicetts/core/tts_engine.py:17-267):
``__init__(config)``, ``synthesize(text, gender, group, area, emotion, sample_iteration,
output_path, reference_audio, reference_text) -> (int16 PCM, seconds)``, context manager,
``cleanup``, ``validate_configuration`` -- and the same host arithmetic in ``_prepare_inputs``
(duration model, chunk plan, frames = samples // hop + 1; :43-131, pinned by golden vectors).

What changes is where the work runs.  The reference walks the chunks one by one and pays
1 + 31 + 1 ``session.run`` host round trips per chunk (:225-238, 157-172).  Here all chunks of a text
(they are independent until the final cross-fade, :244-246) go to the GPU as ONE ragged batch whose
state stays in HBM for all Euler steps; only int16 PCM comes back.  ``_run_preprocess`` /
``_run_transformer_steps`` / ``_run_decode`` remain for reference-style callers and drive the
session objects exactly as the reference does.

Error conventions follow the reference: select_sample errors propagate unwrapped (:217), anything in
the per-chunk work becomes RuntimeError("Speech synthesis failed: ...") (:256-257).  Calls are
serialised by a lock: the REST layer enters from several worker threads (api/tts_engine.py:79-87).
"""
from __future__ import annotations

import logging
import threading
import time
from typing import List, Optional, Tuple

import numpy as np

from .audio_processor import AudioProcessor
from .model import ModelSessionManager
from .model_config import ModelConfig
from .text_processor import TextProcessor
from ..request_options import RequestOptions, column

logger = logging.getLogger("vietvoicetts")


class TTSEngine:
    def __init__(self, config: Optional[ModelConfig] = None, session_factory=None):
        self.config = config or ModelConfig()
        self.model_session_manager = ModelSessionManager(self.config, session_factory=session_factory)
        self.model_session_manager.load_models()
        if self.config.block_cache is not None and self.model_session_manager.spec is not None:      # N23: the span against this model's depth
            from ..model_spec import check_block_cache
            try:
                check_block_cache(self.config.block_cache, self.model_session_manager.spec.depth)
            except ValueError:
                self.model_session_manager.cleanup()
                raise
        if not self.model_session_manager.vocab_path:
            raise RuntimeError("Vocabulary file not found in model tar archive")
        self.text_processor = TextProcessor(self.model_session_manager.vocab_path)
        self.audio_processor = AudioProcessor()
        self.sample_cache = {}
        self.voice_bank = None                    # N3: device-resident reference clips (HIP engine only)
        if self.model_session_manager.engine is not None:
            from ..voice_bank import VoiceBank
            self.voice_bank = VoiceBank(self.model_session_manager.engine, self.config.sample_rate)
        self._lock = threading.Lock()
        self._decode_graphs = None               # DecodeGraphCache, created with the first captured decode (use_hip_graph)
        self._last_plan = []
        self.last_cfg_reuse_report = []          # N21 (config.cfg_reuse_report): the drift reports of the last synthesis, float64 [n_evals, B, 2] per GPU batch
        self.last_block_cache_report = []        # N23 (config.block_cache_report): the reports of the last synthesis, float64 [n_evals, B, 2, 2] per GPU batch
        self.last_cfg_norm_report = []           # N24 (config.cfg_norm_report): the (s, f) of the last synthesis, float32 [n_evals, B, 2] per GPU batch
        self.last_ode_report = []                # N20 (config.ode_report): the step reports of the last synthesis, float64 [n_steps, B, 2] per GPU batch

    def cleanup(self) -> None:
        if self._decode_graphs is not None:       # captured graphs point into the context about to be destroyed, and pin HBM
            self._decode_graphs.clear()
            self._decode_graphs = None
        if self.model_session_manager:
            self.model_session_manager.cleanup()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        self.cleanup()

    # ------------------------------------------------------------------ host arithmetic
    def _chunk_seconds(self, chunk: str, rate: float, speed: float) -> float:
        n = self.text_processor.calculate_text_length(chunk, self.config.pause_punctuation)
        return max(n / rate / speed, self.config.min_target_duration)

    def _prepare_inputs(self, reference_audio_path_or_bytes, reference_text: str, target_text: str,
                        speed: Optional[float] = None) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
        cfg = self.config
        speed = cfg.speed if speed is None else speed
        if getattr(self, "voice_bank", None) is not None:   # decoded / resampled / normalised once on the GPU, then cached in HBM
            audio = self.voice_bank.get(reference_audio_path_or_bytes).pcm_host.reshape(1, 1, -1)
        else:
            audio = self.audio_processor.load_audio(reference_audio_path_or_bytes, cfg.sample_rate).reshape(1, 1, -1)
        reference_text = self.text_processor.clean_text(reference_text)
        target_text = self.text_processor.clean_text(target_text)

        n_samples = audio.shape[-1]
        # The reference admits any clip (core/audio_processor.py:15-26, core/tts_engine.py:46-56) and leaves a too-short one to the
        # preprocess graph.  Its mel front end is a centred STFT, which reflects n_fft / 2 samples at both ends: defined only for
        # clips of more than n_fft / 2 samples.  Refused here, before anything is launched, in the wording of the reference's
        # other reference-audio error (:73); `synthesize` wraps it like every error of the per-chunk work (:256-257).
        spec = getattr(getattr(self, "model_session_manager", None), "spec", None)
        min_samples = (spec.n_fft // 2 + 1) if spec is not None else 1
        if n_samples < min_samples:
            raise ValueError(f"Reference audio is too short ({n_samples} samples, {n_samples / cfg.sample_rate:.3f}s): "
                             f"at least {min_samples} samples ({min_samples / cfg.sample_rate:.3f}s) are needed")
        ref_frames = n_samples // cfg.hop_length + 1
        ref_seconds = n_samples / cfg.sample_rate
        ref_units = self.text_processor.calculate_text_length(reference_text, cfg.pause_punctuation)
        rate = ref_units / ref_seconds if ref_seconds > 0 else 100          # text units per second of the voice
        total = ref_seconds + self._chunk_seconds(target_text, rate, speed)

        if total <= cfg.max_chunk_duration:
            chunks = [target_text]
        else:
            budget = cfg.max_chunk_duration - ref_seconds - 1.0             # 1 s safety margin
            if budget <= 0:
                raise ValueError(f"Reference audio duration ({ref_seconds:.1f}s) exceeds max chunk duration ({cfg.max_chunk_duration}s)")
            chunks = []
            for piece in self.text_processor.chunk_text(target_text, max_chars=int(rate * budget * speed)):
                secs = self._chunk_seconds(piece, rate, speed)
                if ref_seconds + secs <= cfg.max_chunk_duration:
                    chunks.append(piece)
                else:                                                         # still too long: split again, 10 % tighter
                    chunks.extend(self.text_processor.chunk_text(piece, max_chars=int(len(piece) * budget / secs * 0.9)))
            logger.info("Long text (estimated %.1fs) split into %d chunks", total, len(chunks))

        prepared = []
        for piece in chunks:
            secs = self._chunk_seconds(piece, rate, speed)
            frames = ref_frames + int(secs * cfg.sample_rate) // cfg.hop_length + 1
            ids = self.text_processor.text_to_indices([list(reference_text + piece)])
            prepared.append((audio, ids, np.array([frames], dtype=np.int64), np.array([0], dtype=np.int32)))
        return prepared

    # ------------------------------------------------------------------ reference-style stage drivers
    def _run_preprocess(self, audio: np.ndarray, text_ids: np.ndarray, max_duration: np.ndarray):
        m = self.model_session_manager
        names = m.input_names["preprocess"]
        return m.sessions["preprocess"].run(m.output_names["preprocess"], {names[0]: audio, names[1]: text_ids, names[2]: max_duration})

    def _run_transformer_steps(self, noise, rope_cos_q, rope_sin_q, rope_cos_k, rope_sin_k, cat_mel_text, cat_mel_text_drop, time_step):
        m = self.model_session_manager
        names, outs, sess = m.input_names["transformer"], m.output_names["transformer"], m.sessions["transformer"]
        for _ in range(0, self.config.nfe_step - 1, self.config.fuse_nfe):
            noise, time_step = sess.run(outs, dict(zip(names, (noise, rope_cos_q, rope_sin_q, rope_cos_k, rope_sin_k,
                                                               cat_mel_text, cat_mel_text_drop, time_step))))
        return noise, time_step

    def _run_decode(self, noise: np.ndarray, ref_signal_len: np.ndarray) -> np.ndarray:
        m = self.model_session_manager
        names = m.input_names["decode"]
        return m.sessions["decode"].run(m.output_names["decode"], {names[0]: noise, names[1]: ref_signal_len})[0]

    def _device_noise(self) -> bool:
        """N9: the start noise is drawn in HBM (config.noise_source == "device"; the HIP engine only -- injected sessions draw their own)."""
        return self.config.noise_source == "device" and self.model_session_manager.engine is not None

    def _synthesize_sessions(self, inputs_list, noise_keys=None) -> List[np.ndarray]:
        """noise_keys (device noise source): the chunks' key rows; default = a call of its own (the next call serial)."""
        if self._device_noise():
            m = self.model_session_manager
            m.queue_session_keys(m.take_noise_keys(len(inputs_list)) if noise_keys is None else noise_keys)
        waves = []
        for audio, text_ids, max_duration, time_step in inputs_list:
            pre = self._run_preprocess(audio, text_ids, max_duration)
            noise, _ = self._run_transformer_steps(*pre[:7], time_step)
            waves.append(self._run_decode(noise, pre[7]))
        return waves

    # ------------------------------------------------------------------ device-resident batched path
    # ------------------------------------------------------------------ the output stage (N10)
    def _output_options(self) -> Tuple[Optional[int], str]:
        """(output rate or None when it is the model's own, encoding)."""
        cfg = self.config
        rate = cfg.output_sample_rate
        return (None if rate is None or int(rate) == int(cfg.sample_rate) else int(rate)), cfg.output_encoding

    @property
    def output_rate(self) -> int:
        return self._output_options()[0] or self.config.sample_rate

    def _resolved(self, options, n: int) -> List[RequestOptions]:
        """``n`` requests' RequestOptions (None = none has any) with the engine's value in every field they leave open."""
        return [(o or RequestOptions()).resolved(self.config) for o in options or [None] * n]

    def _device_output(self, options=None) -> bool:
        """The chunks stay in HBM until the final bytes exist: asked for by ``output_stage="device"``, and taken on the HIP engine whenever a
        rate, an encoding, a loudness target, a limiter, a pitch, a tempo, a denoiser strength or a watermark key is set: the engine's, or
        the own one of a request of ``options`` (the batch's RequestOptions).  False = today's path: one copy per chunk group, the numpy join."""
        rate, enc = self._output_options()
        return self.model_session_manager.engine is not None and (
            self.config.output_stage == "device" or rate is not None or enc != "pcm16"
            or any(o.wants_output_stage() for o in self._resolved(options, 1)))

    def _denoise_bias_host(self) -> np.ndarray:
        """The bias profile the host mirror subtracts (N19): the caller's ``output_denoise_bias``, else the model's own, which only a HIP
        engine can decode (HipSynth.vocoder_bias; the device's 513 values equal the mirror's bit for bit)."""
        if self.config.output_denoise_bias is not None:
            return np.asarray(self.config.output_denoise_bias, dtype=np.float64)
        eng = self.model_session_manager.engine
        if eng is None:
            raise ValueError("output_denoise without output_denoise_bias needs the HIP engine: the model's bias is what its decoder makes of an "
                             "empty mel; give output_denoise_bias, or unset output_denoise")
        return eng.vocoder_bias()[0].cpu().numpy()

    def _finish_host(self, waves, options: Optional[RequestOptions] = None) -> np.ndarray:
        """One request's chunks -> its final audio on the host: the reference's join, the denoiser's mirror directly behind it (N19), then
        the host mirrors of pitch and tempo (N14, N18), the watermark (N22), the loudness normalisation (N12), the limiter (N13), the
        output rate and the encoding.  ``options`` = the request's own values, None (or a None field) = the engine's."""
        from .audio_processor import encode_output, limit_peaks, normalize_loudness, resample_output, shift_prosody
        cfg, (o,) = self.config, self._resolved([options], 1)
        final = self.audio_processor.concatenate_with_crossfade_improved(waves, cfg.cross_fade_duration, cfg.sample_rate)
        pcm16 = lambda a: np.ascontiguousarray(a, dtype=np.int16)  # noqa: E731
        if o.denoise is not None:
            from .audio_processor import denoise_pcm
            final = denoise_pcm(pcm16(final), self._denoise_bias_host(), o.denoise)
        if o.pitch is not None or o.tempo is not None:
            final = shift_prosody(pcm16(final), o.pitch, o.tempo, formants=o.formants)
        if o.watermark_payload is not None:
            from .audio_processor import watermark_embed
            final = watermark_embed(pcm16(final), cfg.output_watermark_key, o.watermark_payload, cfg.output_watermark_strength)
        if o.loudness is not None:
            final = normalize_loudness(pcm16(final), cfg.sample_rate, o.loudness, cfg.output_peak_dbfs, limiter=o.limiter)
        elif o.limiter is not None:
            final = limit_peaks(pcm16(final), cfg.sample_rate, cfg.output_peak_dbfs, o.limiter)[0]
        rate, enc = self._output_options()
        if rate is not None:
            final = resample_output(final, cfg.sample_rate, rate)
        return encode_output(final, enc, self.output_rate, lpc_order=cfg.flac_lpc_order) if enc != "pcm16" else final

    def _finish_device(self, dev_pcm, counts, options: Optional[List[RequestOptions]] = None) -> List[np.ndarray]:
        """``_synthesize_device(.., device_out=True)``'s result and the number of chunks of each request -> the requests' final audio:
        one HipSynth.finish_output call (join, denoiser, prosody, watermark, loudness, limiter, rate, encoding in HBM; one device-to-host copy).
        ``options`` = per request its own values, None (or a None field) = the engine's.  finish_output reads a column that is None for
        every request as "off" and calls nothing for it."""
        pcm, spans = dev_pcm
        plans, pos = [], 0
        for n in counts:
            plans.append(spans[pos: pos + n])
            pos += n
        cfg = self.config
        opts = self._resolved(options, len(counts))
        rate, enc = self._output_options()
        mark = {}
        if cfg.output_watermark_key is not None:          # N22: the column travels only with a key; without one the call is the one of ever
            mark = dict(watermark=column(opts, "watermark_payload"), watermark_key=cfg.output_watermark_key,
                        watermark_strength=cfg.output_watermark_strength)
        return self.model_session_manager.engine.finish_output(
            pcm, plans, cfg.cross_fade_duration, cfg.sample_rate, rate, enc, peak_dbfs=cfg.output_peak_dbfs, flac_lpc_order=cfg.flac_lpc_order,
            denoise_bias=cfg.output_denoise_bias, **{name: column(opts, name) for name in ("loudness", "limiter", "pitch", "tempo", "formants", "denoise")},
            **mark)

    def _set_ode_plan(self) -> None:
        """The solver and its step report as the config has them now (the report is off while the plan changes under it)."""
        eng = self.model_session_manager.engine
        eng.set_ode_report(False)
        eng.set_nfe(self.config.nfe_step, self.config.ode_method, self.config.cfg_zero_init)
        eng.set_ode_report(self.config.ode_report)
        eng.set_cfg_norm_report(self.config.cfg_norm_report)
        eng.set_cfg_reuse_report(self.config.cfg_reuse_report)
        eng.set_block_cache_report(self.config.block_cache_report)

    def _synthesize_device(self, inputs_list, noise_blocks=None, noise_keys=None, device_out: bool = False, options=None):
        """inputs_list items are (audio (1,1,S_i), text_ids (1,T_i), max_duration (1,), time_step); the reference
        clips may differ per item (cross-request batches).  One ragged GPU batch per ``max_batch_chunks`` items.
        noise_blocks: optional pre-drawn (N_i, n_mel) fp32 tensors, one per item (the batching front end draws them from
        per-request generators); default = the manager's seeded stream, in item order, like the session path.
        noise_keys (N9, ``noise_source="device"``): uint64 [n_items][2] Philox key rows (model_spec.noise_keys), one per item: the noise is
        drawn in HBM by vv_noise_fill, no host tensor is built and none is uploaded.  Default with that source = a call of its own (the
        next call serial); explicit noise_blocks still win.
        options: optional RequestOptions per item (None, a None entry or a None field = the engine's value), read for the acoustic stage:
        ``cfg_strength`` (None in the config as well leaves it to the model); ``cfg_interval`` (lo, hi): an item is guided at the evaluations
        inside its interval, and never when its strength is 0: elsewhere its unconditional branch is not computed; ``apg_eta`` /
        ``apg_norm``: items with neither keep the plain combine, in the same batch; ``cfg_zero_star`` / ``cfg_rescale`` (N24): the call goes to
        vv_transformer_steps_norm only when some item of it has either, and items with neither keep the plain combine there.
        device_out (N10): nothing is copied to the host; returns (int16 device tensor, [(offset, samples) per item]) -- the planes of the
        chunk groups back to back and each item's span in them, the lengths from the host's own frame counts (no readback)."""
        import torch
        m = self.model_session_manager
        eng, spec = m.engine, m.spec
        dev = eng.device
        self._set_ode_plan()
        self.last_ode_report = []
        self.last_cfg_reuse_report = []
        self.last_block_cache_report = []
        self.last_cfg_norm_report = []
        hop = self.config.hop_length
        opts = self._resolved(options, len(inputs_list))
        star_all, resc_all = ([getattr(o, name) for o in opts] for name in ("cfg_zero_star", "cfg_rescale"))
        g_all, iv_all, eta_all, norm_all, reuse_all = ([getattr(o, name) for o in opts]
                                                       for name in ("cfg_strength", "cfg_interval", "apg_eta", "apg_norm", "cfg_reuse"))
        from ..model_spec import check_apg, check_cfg_norm, check_cfg_norm_combination
        apg_on = [check_apg(e, r) is not None for e, r in zip(eta_all, norm_all)]
        norm_on = [check_cfg_norm(z, r) is not None for z, r in zip(star_all, resc_all)]
        for j in range(len(opts)):                           # N24: never with APG, reuse or the block-cache entry, each in its own words
            check_cfg_norm_combination(star_all[j], resc_all[j], eta_all[j], norm_all[j], reuse_all[j], self.config.block_cache)
        for k, on in zip(reuse_all, apg_on):
            if (k or 1) > 1 and on:
                raise ValueError("cfg_reuse > 1 cannot be combined with apg_eta / apg_norm (projected guidance needs both predictions at every evaluation)")
        # N23: the engine's block caching for every batch.  Its entry takes no mask: a request's strength travels per item (also a strength
        # of 0, whose unconditional rows are then computed and weighted by 0), and a request with an interval, reuse or APG of its own is refused
        bc = dict(block_cache=self.config.block_cache, block_cache_interval=self.config.block_cache_interval)
        if self.config.block_cache is not None and (any(v is not None for v in iv_all) or any((k or 1) > 1 for k in reuse_all) or any(apg_on)):
            raise ValueError("block_cache cannot be combined with a request's cfg_interval, cfg_reuse > 1 or apg_eta / apg_norm")
        from ..sharding import plan_batches
        n_items = len(inputs_list)
        seq_all = [int(g[2][0]) for g in inputs_list]
        if noise_blocks is not None:
            noise_keys = None
        elif noise_keys is not None or self._device_noise():
            noise_keys = m.take_noise_keys(n_items) if noise_keys is None else np.asarray(noise_keys, dtype=np.uint64).reshape(-1, 2)
            if len(noise_keys) != n_items:
                raise ValueError(f"{len(noise_keys)} noise key rows for {n_items} items")
        else:                         # the same seeded stream the session path draws from: one (N_i, n_mel) block per chunk, in item order
            noise_keys = None
            noise_blocks = [torch.randn((n, spec.n_mel), generator=m.noise_gen, dtype=torch.float32) for n in seq_all]
        waves: List[Optional[np.ndarray]] = [None] * n_items
        planes, spans, plane_base = [], [None] * n_items, 0
        # the device packs ragged rows, so padding is free for the acoustic stages; sorting by length still puts similar
        # lengths into the same batch when a text has more chunks than max_batch_chunks (vocoder planes are padded)
        groups = []
        row_cap = eng.max_rows_per_call()          # the packed qkv buffer of one call stays below 2 GiB
        for idx in plan_batches(seq_all, max(1, int(self.config.max_batch_chunks)), pad_frac=1.0):
            cur, rows = [], 0
            for i in idx:
                if cur and rows + seq_all[i] > row_cap:
                    groups.append(cur)
                    cur, rows = [], 0
                cur.append(i)
                rows += seq_all[i]
            groups.append(cur)
        # N21: a call either reuses guidance differences or projects them (APG); items of the two kinds of one group run as two calls (every
        # kernel of the path is row- or sequence-local, so an item's audio does not depend on which call it sits in)
        groups = [part for idx in groups
                  for part in (([[i for i in idx if (reuse_all[i] or 1) > 1], [i for i in idx if not (reuse_all[i] or 1) > 1]]
                                if any(apg_on[i] for i in idx) and any((reuse_all[i] or 1) > 1 for i in idx) else [idx])) if part]
        # N24: a call with CFG-Zero* / rescale takes neither APG nor reuse: such items of one group run as a call of their own
        groups = [part for idx in groups
                  for part in (([[i for i in idx if norm_on[i]], [i for i in idx if not norm_on[i]]]
                                if any(norm_on[i] for i in idx) and any(apg_on[i] or (reuse_all[i] or 1) > 1 for i in idx) else [idx])) if part]
        for idx in groups:
            group = [inputs_list[i] for i in idx]
            B = len(group)
            lens_a = np.array([g[0].shape[-1] for g in group], dtype=np.int32)
            lens_t = np.array([g[1].shape[1] for g in group], dtype=np.int32)
            # the audio plane is at least n_fft wide (vv_preprocess's contract): a lone clip of n_fft/2 + 1 ... n_fft - 1 samples is
            # admitted by _prepare_inputs, its zeros past audio_len are never read (the mel front end reflects inside audio_len)
            S, T = max(int(lens_a.max()), int(spec.n_fft)), int(lens_t.max())
            ids = np.zeros((B, T), dtype=np.int32)
            for i, g in enumerate(group):
                ids[i, : lens_t[i]] = g[1][0]
            banked = [self.voice_bank.entry_for_host(g[0]) if self.voice_bank is not None else None for g in group]
            if all(e is not None for e in banked):               # clips already live in HBM: assemble the batch device-side
                audio = torch.zeros((B, S), dtype=torch.int16, device=dev)
                for i, e in enumerate(banked):
                    audio[i, : lens_a[i]] = e.pcm_dev
            else:
                audio_np = np.zeros((B, S), dtype=np.int16)
                for i, g in enumerate(group):
                    audio_np[i, : lens_a[i]] = g[0].reshape(-1)
                audio = torch.from_numpy(audio_np).to(dev)
            seq = np.array([seq_all[i] for i in idx], dtype=np.int32)
            ref_frames = lens_a // hop + 1
            N = int(seq.max())
            t_gen = int((seq - ref_frames).max())
            if self.config.use_hip_graph:
                # fixed buckets (frames to multiples of 128, generated frames to multiples of 64) so that one captured vocoder graph
                # serves every chunk group and nearby reference-clip lengths; the decode masks every item by its own lengths
                from ..runtime import DecodeGraphCache
                Nb = DecodeGraphCache.bucket(N, 0)[0]
                N, t_gen = DecodeGraphCache.bucket(Nb, Nb - int(ref_frames.min()))      # every chunk group of a text lands on one key
            if noise_keys is None:
                noise = torch.zeros((B, N, spec.n_mel), dtype=torch.float32)
                for i, j in enumerate(idx):
                    noise[i, : seq[i]] = noise_blocks[j]
                keys = None
            else:
                noise, keys = None, eng.noise_keys_device(noise_keys[list(idx)])
            t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
            cfg = None                                   # per-item guidance strength: only when some item asks for one
            if any(g_all[j] is not None for j in idx):
                cfg = torch.tensor([float(spec.cfg_strength) if g_all[j] is None else g_all[j] for j in idx], dtype=torch.float32).to(dev)
            guide = eng.guidance_mask([iv_all[j] for j in idx], [g_all[j] for j in idx], [reuse_all[j] for j in idx])     # None: every item guided everywhere
            apg = eng.apg_tensors([eta_all[j] for j in idx], [norm_all[j] for j in idx])      # None: the plain combine for every item
            cfg_norm = eng.cfg_norm_tensors([star_all[j] for j in idx], [resc_all[j] for j in idx])      # None: no item of the call has either
            if self.config.block_cache is not None:
                guide = None
            if self.config.use_hip_graph:
                pre = eng.preprocess(audio, t32(lens_a), t32(ids), t32(lens_t), t32(seq), N, seq_len_host=seq, audio_len_host=lens_a)
                x = noise.to(dev) if keys is None else eng.noise(keys, pre["seq_len"], N)
                eng.transformer_steps(x, pre, 0, eng.n_steps, cfg=cfg, guide=guide, apg=apg, cfg_norm=cfg_norm, **bc)
                if self._decode_graphs is None:
                    self._decode_graphs = DecodeGraphCache(eng, self.config.decode_graph_cache_entries, self.config.decode_graph_cache_bytes)
                pcm, pcm_len = self._decode_graphs.get(B, N, t_gen)(x, pre["ref_signal_len"], pre["seq_len"])
            else:
                _x, pcm, pcm_len, _pre = eng.synthesize_batch(audio, t32(lens_a), t32(ids), t32(lens_t), t32(seq), N,
                                                              None if noise is None else noise.to(dev), t_gen,
                                                              gen_frames=[int(v) for v in (seq - ref_frames)], seq_len_host=seq,
                                                              audio_len_host=lens_a, cfg=cfg, guide=guide, noise_keys=keys, apg=apg, cfg_norm=cfg_norm, **bc)
            if self.config.cfg_norm_report and cfg_norm is not None:
                self.last_cfg_norm_report.append(eng.last_cfg_norm_report())
            if self.config.ode_report:
                self.last_ode_report.append(eng.last_ode_report())
            if self.config.cfg_reuse_report:
                self.last_cfg_reuse_report.append(eng.last_cfg_reuse_report())
            if self.config.block_cache_report:
                self.last_block_cache_report.append(eng.last_block_cache_report())
            if device_out:
                pcm = pcm.clone() if self.config.use_hip_graph else pcm.contiguous()      # a captured graph's output buffer is replayed over
                for i, j in enumerate(idx):
                    spans[j] = (plane_base + i * pcm.shape[1], spec.pcm_samples(int(seq[i] - ref_frames[i])))
                planes.append(pcm.reshape(-1))
                plane_base += pcm.numel()
                continue
            pcm, pcm_len = pcm.cpu().numpy(), pcm_len.cpu().numpy()
            for i, j in enumerate(idx):
                waves[j] = pcm[i, : pcm_len[i]].reshape(1, 1, -1)
        if device_out:
            return (planes[0] if len(planes) == 1 else torch.cat(planes)), spans
        return waves

    # ------------------------------------------------------------------ public API
    def synthesize(self, text: str, gender: Optional[str] = None, group: Optional[str] = None, area: Optional[str] = None,
                   emotion: Optional[str] = None, sample_iteration: Optional[int] = None, output_path: Optional[str] = None,
                   reference_audio: Optional[str] = None, reference_text: Optional[str] = None) -> Tuple[np.ndarray, float]:
        start = time.time()
        speed = self.config.speed      # read once: the REST layer mutates config.speed around the call (api/tts_engine.py:68-91)
        ref_audio, ref_text = self.model_session_manager.select_sample(gender, group, area, emotion, sample_iteration,
                                                                       reference_audio, reference_text)
        try:
            with self._lock:
                inputs_list = self._prepare_inputs(ref_audio, ref_text, text, speed=speed)
                self._last_plan = [int(i[2][0]) for i in inputs_list]
                if self.model_session_manager.engine is not None:
                    keys = self.model_session_manager.take_noise_keys(len(inputs_list)) if self._device_noise() else None
                    if self._device_output():
                        dev_pcm = self._synthesize_device(inputs_list, noise_keys=keys, device_out=True)
                        waves, final_wave = None, self._finish_device(dev_pcm, [len(inputs_list)])[0]
                    else:
                        waves = self._synthesize_device(inputs_list, noise_keys=keys)
                else:
                    waves = self._synthesize_sessions(inputs_list)
            if waves is not None:
                final_wave = self._finish_host(waves)
            generation_time = time.time() - start
            if output_path:
                self.audio_processor.save_audio(final_wave, output_path, self.output_rate, self.config.output_encoding)
                logger.info("Audio saved to: %s", output_path)
            return final_wave, generation_time
        except Exception as e:
            raise RuntimeError(f"Speech synthesis failed: {str(e)}")

    def synthesize_stream(self, text: str, gender: Optional[str] = None, group: Optional[str] = None, area: Optional[str] = None,
                          emotion: Optional[str] = None, sample_iteration: Optional[int] = None,
                          reference_audio: Optional[str] = None, reference_text: Optional[str] = None, chunks_per_step: int = 1):
        """Generator of PCM blocks (int16 at the output rate, uint8 G.711 codes, the bytes of a FLAC stream: N15, or raw IMA ADPCM blocks: N25): audio is emitted as soon as a group of ``chunks_per_step``
        chunks is synthesised instead of after the whole text (the reference buffers everything, api/app.py:59-65).
        Overlap-save: the improved cross-fade only rewrites the last ``cross_fade_duration`` of what has been joined
        so far (audio_processor.py:122-192), so everything before that tail is final and can be yielded.  The joiner
        (``CrossfadeStream``) keeps only that tail: each raw chunk is clip-repaired once, emitted samples are never
        revisited, and the concatenation of all yielded blocks equals ``synthesize(text)`` sample for sample.
        With ``output_loudness`` set the call raises ValueError at once (N12): an integrated loudness is a property of the WHOLE utterance.
        ``output_limiter`` alone streams (N13): a LimiterStream in front of the output rate / encoding holds back 2L + H samples.
        ``output_pitch`` / ``output_tempo`` raise ValueError at once as well (N14): every frame position depends on the whole past.
        ``output_denoise`` (N19) raises ValueError at once too: there is no block-wise denoiser yet.  So does ``output_watermark_key``
        (N22): the mark is laid on the frames of the whole utterance."""
        if self.config.output_watermark_key is not None:  # N22: the same frames as the denoiser's; there is no block-wise embedder
            raise ValueError("synthesize_stream cannot honour output_watermark_key: the watermark is embedded in the whole utterance; use "
                             "synthesize, or unset output_watermark_key")
        if self.config.output_denoise is not None:        # N19: frames reach 768 samples back; a block-wise DenoiseStream does not exist yet
            raise ValueError("synthesize_stream cannot honour output_denoise: the denoiser works on the whole joined utterance; use "
                             "synthesize, or unset output_denoise")
        if self.config.output_pitch is not None or self.config.output_tempo is not None:
            raise ValueError("synthesize_stream cannot honour output_pitch / output_tempo: the chain of frame positions needs the whole "
                             "utterance; use synthesize, or unset them")
        if self.config.output_loudness is not None:       # checked here, not inside the generator: the caller hears of it without iterating
            raise ValueError("synthesize_stream cannot honour output_loudness: the integrated measure needs the whole utterance; "
                             "use synthesize, or unset output_loudness")
        return self._stream_blocks(text, gender, group, area, emotion, sample_iteration, reference_audio, reference_text, chunks_per_step)

    def _stream_blocks(self, text, gender, group, area, emotion, sample_iteration, reference_audio, reference_text, chunks_per_step):
        """The generator behind ``synthesize_stream``."""
        speed = self.config.speed
        ref_audio, ref_text = self.model_session_manager.select_sample(gender, group, area, emotion, sample_iteration,
                                                                       reference_audio, reference_text)
        try:
            with self._lock:
                inputs_list = self._prepare_inputs(ref_audio, ref_text, text, speed=speed)
                # device noise: ONE call serial for the whole stream, chunk c under it whatever group it is synthesised in
                keys = self.model_session_manager.take_noise_keys(len(inputs_list)) if self._device_noise() else None
            self._last_plan = [int(i[2][0]) for i in inputs_list]
            from .audio_processor import AdpcmStream, CrossfadeStream, FlacStream, LimiterStream, OutputStream
            cfg, eng = self.config, self.model_session_manager.engine
            joiner = CrossfadeStream(len(inputs_list), cfg.cross_fade_duration, cfg.sample_rate)
            # The stages behind the join, in order; each carries the state it needs (on the HIP engine its back end is the device kernel,
            # blocks re-uploaded), so that the blocks still add up to synthesize()'s result
            rate, enc = self._output_options()
            stages = []
            if cfg.output_limiter is not None:                 # N13: finite look-ahead
                backend = None if eng is None else eng.limiter_stream_backend(cfg.sample_rate, cfg.output_peak_dbfs, cfg.output_limiter)
                stages.append(LimiterStream(cfg.sample_rate, cfg.output_peak_dbfs, cfg.output_limiter, backend))
            if rate is not None or enc != "pcm16":             # N10: the filter's position and history
                resample, encode = eng.output_stream_backends(cfg.sample_rate, rate, enc) if eng is not None else (None, None)
                if enc not in ("flac", "adpcm"):
                    stages.append(OutputStream(cfg.sample_rate, rate, enc, resample, encode))
                else:                                          # N15, N25: frames / blocks are independent -- their stream behind the rate conversion
                    if rate is not None:
                        stages.append(OutputStream(cfg.sample_rate, rate, "pcm16", resample, None))
                    stages.append(FlacStream(self.output_rate, encode, lpc_order=cfg.flac_lpc_order) if enc == "flac" else
                                  AdpcmStream(self.output_rate, encode))

            def through(block, stages):                        # handed over as contiguous int16, which PCM blocks are already
                for stage in stages:
                    block = stage.push(np.ascontiguousarray(block, dtype=np.int16))
                return block
            step = max(1, int(chunks_per_step))
            for lo in range(0, len(inputs_list), step):
                with self._lock:
                    if self.model_session_manager.engine is not None:
                        waves = self._synthesize_device(inputs_list[lo: lo + step], noise_keys=None if keys is None else keys[lo: lo + step])
                    else:
                        waves = self._synthesize_sessions(inputs_list[lo: lo + step])
                blocks = [joiner.push(w) for w in waves]
                block = through(np.concatenate(blocks) if len(blocks) > 1 else blocks[0], stages)
                if block.size:
                    yield block
            for k, stage in enumerate(stages):                 # a stage's tail goes through the stages behind it, which are flushed in turn
                block = through(stage.flush(), stages[k + 1:])
                if block.size:
                    yield block
        except Exception as e:
            raise RuntimeError(f"Speech synthesis failed: {str(e)}")

    def edit_speech(self, audio, text: str, parts_to_edit, fix_duration=None, seed: Optional[int] = None,
                    output_path: Optional[str] = None) -> Tuple[np.ndarray, float]:
        """Speech editing (F5-TTS speech_edit.py): regenerate the spans ``parts_to_edit`` = [(start, end)] seconds of
        ``audio`` (a path or WAV bytes, taken in like a reference clip, or an int16 array at ``config.sample_rate``) so that the clip
        says ``text`` (the corrected FULL transcript); ``fix_duration`` = the new length of each span in seconds (default: unchanged).
        Only the spans are drawn from noise; every other frame conditions the model and is put back after the last step, and the
        whole clip is rendered again by the vocoder.  Noise: the manager's seeded stream, or ``torch.Generator().manual_seed(seed)``; with
        ``noise_source="device"`` the Philox stream (seed or random_seed, edit serial, edit=True) of model_spec.noise_keys.
        Returns (int16 PCM of the spliced length -- hop * (N - 1) samples of it with the Vocos decoder --, seconds).  Validation errors propagate as ValueError; device failures become
        RuntimeError("Speech editing failed: ...")."""
        import torch
        from ..pack import MAX_POS
        from ..speech_edit import plan_edit
        start = time.time()
        m = self.model_session_manager
        eng = m.engine
        if eng is None:
            raise RuntimeError("Speech editing runs on the HIP engine only: the session IO of the reference graphs has no frame mask")
        cfg = self.config
        sr, hop = cfg.sample_rate, cfg.hop_length
        if not isinstance(audio, (str, bytes, bytearray)):
            audio = self.audio_processor.to_wav_bytes(np.asarray(audio, dtype=np.int16), sr)
        clean = self.text_processor.clean_text(text)
        if not clean.strip(" .,?!"):                  # clean_text ends every text with a punctuation mark
            raise ValueError("the transcript of the edited clip is empty")
        with self._lock:
            entry = self.voice_bank.get(bytes(audio) if isinstance(audio, bytearray) else audio)
            plan = plan_edit(entry.n_samples, parts_to_edit, fix_duration, sr, hop, m.spec.n_fft, MAX_POS)
            if plan.spliced_len / sr > cfg.max_chunk_duration:
                raise ValueError(f"the edited clip would last {plan.spliced_len / sr:.2f}s, more than max_chunk_duration "
                                 f"({cfg.max_chunk_duration}s)")
            if self._device_noise():      # N9: edits have streams of their own (bit 63); a given seed is serial 0 -- the call is reproducible
                from ..model_spec import noise_keys
                noise, keys = None, (m.take_edit_keys() if seed is None else noise_keys(int(seed), 0, 1, edit=True))
            else:
                gen = m.noise_gen if seed is None else torch.Generator().manual_seed(int(seed))
                noise, keys = torch.randn((plan.n_frames, m.spec.n_mel), generator=gen, dtype=torch.float32), None
            ids = self.text_processor.text_to_indices([list(clean)])
            try:
                dev = eng.device
                self._set_ode_plan()
                g_item = None if cfg.cfg_strength is None else torch.full((1,), float(cfg.cfg_strength), dtype=torch.float32, device=dev)
                _x, pcm, n_out = eng.edit_batch(entry.pcm_dev, plan.rows(), [plan.spliced_len],
                                               torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev),
                                               torch.tensor([ids.shape[1]], dtype=torch.int32, device=dev),
                                               torch.from_numpy(plan.keep.reshape(1, -1)).to(dev),
                                               None if noise is None else noise.unsqueeze(0).to(dev), cfg=g_item,
                                               guide=None if cfg.block_cache is not None else eng.guidance_mask(cfg.cfg_interval, [cfg.cfg_strength], cfg.cfg_reuse),
                                               noise_keys=keys, apg=eng.apg_tensors([cfg.apg_eta], [cfg.apg_norm]), block_cache=cfg.block_cache,
                                               block_cache_interval=cfg.block_cache_interval,
                                               cfg_norm=eng.cfg_norm_tensors([cfg.cfg_zero_star], [cfg.cfg_rescale]))
                self.last_cfg_norm_report = [eng.last_cfg_norm_report()] if cfg.cfg_norm_report else []
                self.last_ode_report = [eng.last_ode_report()] if cfg.ode_report else []
                self.last_cfg_reuse_report = [eng.last_cfg_reuse_report()] if cfg.cfg_reuse_report else []
                self.last_block_cache_report = [eng.last_block_cache_report()] if cfg.block_cache_report else []
                if self._device_output():                         # N10: rate / encoding in HBM; the length from the host's own plan
                    n_host = min(plan.spliced_len, m.spec.pcm_samples(plan.n_frames))
                    wave = self._finish_device((pcm[0], [(0, n_host)]), [1])[0]      # one request of one span, the engine's options
                else:
                    wave = pcm[0, : int(n_out[0])].cpu().numpy()      # the spliced length (HiFi-GAN); hop * (N - 1) <= it (Vocos)
            except Exception as e:
                raise RuntimeError(f"Speech editing failed: {str(e)}") from e
        if output_path:
            self.audio_processor.save_audio(wave, output_path, self.output_rate, cfg.output_encoding)
            logger.info("Audio saved to: %s", output_path)
        return wave, time.time() - start

    def detect_watermark(self, audio, key: Optional[int] = None):
        """Look for this engine's watermark in ``audio``: a path or the bytes of a WAV or FLAC file (any rate and channel
        count, taken in like a reference clip: mono at ``config.sample_rate``), or an int16 array at that rate; a list of those is
        answered with a list, from one device call for all clips.  ``key`` = None: the engine's ``output_watermark_key``.  On the HIP
        engine the statistic is vv_pcm_watermark_detect's, else the host mirror's (equal, bit for bit).
        -> audio_processor.WatermarkResult: score, present, offset (the alignment in hops), payload (None unless crc_ok), crc_ok, z."""
        from .audio_processor import WATERMARK_DETECT_MAX_N, check_watermark_key, watermark_decide, watermark_stats
        key = check_watermark_key(self.config.output_watermark_key if key is None else key)
        if key is None:
            raise ValueError("detect_watermark needs a key: give one, or set output_watermark_key")
        many = isinstance(audio, (list, tuple))
        clips = []
        for a in (audio if many else [audio]):
            if isinstance(a, (str, bytes, bytearray)):
                a = self.audio_processor.load_audio(bytes(a) if isinstance(a, bytearray) else a, self.config.sample_rate)
            a = np.ascontiguousarray(np.asarray(a).reshape(-1))
            if a.dtype != np.int16 or a.size > WATERMARK_DETECT_MAX_N:
                raise ValueError(f"detect_watermark: int16 PCM of at most {WATERMARK_DETECT_MAX_N} samples expected")
            clips.append(a)
        if not clips:
            return []
        eng = self.model_session_manager.engine
        if eng is None:
            out = [watermark_decide(watermark_stats(a, key)) for a in clips]
        else:
            import torch
            from ..pcm_stage import _place
            offs, end = _place([a.size for a in clips], 8)
            flat = np.zeros(max(end, 8), np.int16)
            for o, a in zip(offs, clips):
                flat[o: o + a.size] = a
            with self._lock:
                stats = eng.pcm_watermark_detect(torch.from_numpy(flat).to(eng.device), [[o, a.size] for o, a in zip(offs, clips)], key).cpu().numpy()
            out = [watermark_decide(s) for s in stats]
        return out if many else out[0]

    def validate_configuration(self, reference_audio: Optional[str] = None) -> bool:
        if reference_audio is None:
            return True          # built-in voice samples are used
        return self.config.validate_with_reference_audio(reference_audio)
