"""ModelConfig -- the knobs of the synthesis engine, field-for-field compatible with the reference
(vietvoicetts/core/model_config.py:21-63: names, defaults, validation ranges, dict round trip
:143-153, alias TTSConfig :157, MODEL_* constants :15-18).

Differences, all additive:
  * there is no network here, so nothing is ever downloaded: ``ensure_model_downloaded`` returns
    the cached model pack if it exists, builds a SYNTHETIC pack when ``synthetic_model`` (or the
    env var VIETVOICE_TTS_SYNTHETIC=1) asks for one, and otherwise raises the same RuntimeError
    family the reference raises when its download fails (model_config.py:93-100, 106-112);
  * build-only fields (device, acoustic_dtype, model_spec, ...) with defaults, so
    ``ModelConfig(**reference_dict)`` keeps working.
The onnxruntime knobs are kept as inert fields for API compatibility.
"""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Optional, Sequence, Tuple

logger = logging.getLogger("vietvoicetts")

MODEL_GENDER = ["male", "female"]
MODEL_GROUP = ["story", "news", "audiobook", "interview", "review"]
MODEL_AREA = ["northern", "southern", "central"]
MODEL_EMOTION = ["neutral", "serious", "monotone", "sad", "surprised", "happy", "angry"]


@dataclass
class ModelConfig:
    # --- reference fields (same order, names and defaults)
    model_url: str = "https://huggingface.co/nguyenvulebinh/VietVoice-TTS/resolve/main/model-bin.pt"
    model_cache_dir: str = "models"
    model_filename: str = "model-bin.pt"
    nfe_step: int = 32
    fuse_nfe: int = 1
    sample_rate: int = 24000
    speed: float = 0.9
    random_seed: int = 9527
    hop_length: int = 256
    gender: Optional[str] = "female"
    area: Optional[str] = "northern"
    emotion: Optional[str] = "neutral"
    group: Optional[str] = "audiobook"
    pause_punctuation: str = r".,?!:"
    cross_fade_duration: float = 0.1
    max_chunk_duration: float = 20.0
    min_target_duration: float = 1.0
    log_severity_level: int = 4
    log_verbosity_level: int = 4
    inter_op_num_threads: int = 0
    intra_op_num_threads: int = 0
    enable_cpu_mem_arena: bool = True
    # --- build-only fields
    device: str = "cuda:0"
    acoustic_dtype: str = "bf16"            # "bf16" (throughput) or "fp32" (numerics configuration)
    synthetic_model: bool = False           # build a seeded synthetic model pack when none is cached
    model_spec: str = "full"                # architecture preset of a synthetic pack: full | small | tiny (+ "-vocos")
    max_batch_chunks: int = 32              # chunks of one long text synthesised per GPU batch
    use_hip_graph: bool = False             # replay the vocoder step from a captured hipGraph (fixed frame buckets)
    decode_graph_cache_entries: int = 8     # captured decode graphs kept per engine (least recently used beyond that)
    decode_graph_cache_bytes: int = 16 << 30   # HBM the cache may pin (shared workspace + per-graph I/O buffers)
    ode_method: str = "euler"               # flow-ODE solver: euler | midpoint | heun2 | heun3 | rk4 (model_spec.ODE_METHODS); nfe_step stays
                                            # the number of grid points, the DiT runs stages x (nfe_step - 1) times.  Or ab2 | ab3
                                            # (model_spec.ODE_MULTISTEP): Adams-Bashforth on the slopes of the steps before,
                                            # nfe_step - 1 evaluations as euler
    ode_report: bool = False                # N20, needs ab2 | ab3: per step and item the sums (|f_n - f_{n-1}|^2, |f_n|^2) of the combined velocity,
                                            # reduced on the device -- the local-error term of the Euler step (HipSynth.last_ode_report,
                                            # TTSEngine.last_ode_report).  Off = nothing is launched or allocated for it
    cfg_strength: Optional[float] = None    # classifier-free guidance strength of every synthesis of this engine; None = the model's
    cfg_interval: Optional[Tuple[float, float]] = None   # guidance only at the evaluations with lo <= t <= hi (limited-interval guidance);
                                            # outside it the unconditional branch is not computed.  None = guidance everywhere
    apg_eta: Optional[float] = None         # adaptive projected guidance (model_spec.check_apg): the factor on the part of the guidance difference
                                            # parallel to the conditional data estimate (0 removes it, 1 or None = plain CFG)
    apg_norm: Optional[float] = None        # ... and the cap on the RMS of the data-space guidance difference (None = no cap)
    cfg_reuse: Optional[int] = None         # guidance reuse: the unconditional branch runs at every k-th guided evaluation of an item
                                            # only; in between the stored guidance difference p_c - p_u is combined with the fresh p_c.  None or 1 =
                                            # off (every guided evaluation computes both).  Not combined with apg_eta / apg_norm
    cfg_reuse_report: bool = False          # N21, needs cfg_reuse > 1: per evaluation and item the sums (|D - D_stored|^2, |D|^2) of the guidance
                                            # difference at the computed evaluations, reduced on the device -- how far it moved while it was reused
                                            # (HipSynth.last_cfg_reuse_report, TTSEngine.last_cfg_reuse_report).  Off = nothing is launched or allocated
    block_cache: Optional[Tuple[int, int, int]] = None      # block caching, (first, last, every): the DiT blocks [first, last) run at
                                            # every ``every``-th evaluation only; in between their stored contribution to the residual stream is added
                                            # back instead.  None, or every = 1 = off.  The span is checked against the model's depth when the engine is
                                            # built.  Not combined with cfg_interval, cfg_reuse > 1 or apg_eta / apg_norm
    block_cache_interval: Optional[Tuple[float, float]] = None   # ... only at the evaluations with lo <= t <= hi; None = everywhere.  Needs block_cache
    block_cache_report: bool = False        # N23, needs block_cache: per evaluation, item and CFG branch the sums (|C - C_stored|^2, |C|^2) of the span's
                                            # contribution at the full evaluations, reduced on the device -- how far it moved while it was reused
                                            # (HipSynth.last_block_cache_report, TTSEngine.last_block_cache_report).  On, every full evaluation stores
    cfg_zero_star: bool = False             # CFG-Zero* (Fan et al. 2025): a guided item's unconditional velocity is scaled by the per-item
                                            # s* = <p_c, p_u> / <p_u, p_u> before the combine.  Not combined with apg_eta / apg_norm, cfg_reuse > 1 or block_cache
    cfg_rescale: Optional[float] = None     # guidance rescale phi, 0 < phi <= 1 (N24; Lin et al. 2024, on the guided velocity): the guided slope is scaled
                                            # by phi std(p_c) / std(k) + 1 - phi per item.  None = off.  Same refusals as cfg_zero_star
    cfg_zero_init: int = 0                  # zero-init (N24): the first K ODE steps are skipped -- the state stays the start noise up to t_K and their
                                            # DiT evaluations are not run.  0 <= K <= nfe_step - 2; engine-wide, as ode_method
    cfg_norm_report: bool = False           # N24, needs cfg_zero_star or cfg_rescale: the (s, f) every evaluation used, per item
                                            # (HipSynth.last_cfg_norm_report, TTSEngine.last_cfg_norm_report).  Off = nothing is allocated for it
    noise_source: str = "host"              # where the flow ODE's start noise is drawn: "host" = torch.randn from seeded generators, uploaded;
                                            # "device" = Philox4x32-10 in HBM keyed by (random_seed, call serial, chunk) -- model_spec.noise_keys
    output_stage: str = "host"              # where the chunks of a text are joined: "host" = numpy after one copy per chunk group (the reference's
                                            # function); "device" = vv_join_chunks in HBM, bit for bit the same samples, one copy of the final bytes
    output_sample_rate: Optional[int] = None   # None = sample_rate; else the output is rate-converted (band-limited polyphase FIR, vv_pcm_resample)
    output_encoding: str = "pcm16"          # "pcm16" | "ulaw" | "alaw" (G.711, uint8 codes, vv_pcm_encode) | "flac" (a FLAC file, lossless, vv_pcm_flac: N15).  A rate or an encoding runs on the
                                            # device on the HIP engine, through the host mirrors on injected sessions.
                                            # "adpcm" (N25, vv_pcm_adpcm): an IMA ADPCM WAVE file, format tag 0x11, 4 bits per sample, blocks of 256 bytes per
                                            # 11025 Hz of the output rate; synthesize_stream yields the raw blocks (adpcm_wav makes a file of them)
    flac_lpc_order: int = 0                 # highest LPC order the FLAC encoder tries per frame, 1 ... 12 (vv_pcm_flac_lpc): smaller files on
                                            # tonal material, the same samples back.  0 = fixed predictors only, the encoder of N15 byte for byte.  Needs
                                            # output_encoding "flac"
    output_loudness: Optional[float] = None  # programme loudness of every utterance in LUFS (ITU-R BS.1770-4 integrated, gated), -60 ... -5; None = off.
                                            # Measured and applied after the join, before the output rate and the encoding (vv_pcm_loudness on the HIP
                                            # engine, audio_processor.normalize_loudness on injected sessions).  Not available in synthesize_stream
    output_peak_dbfs: float = -1.0          # sample-peak ceiling of the loudness gain in dBFS, -20 ... 0 (no oversampled true peak)
    output_limiter: Optional[str] = None    # None | "sample" | "true": a look-ahead limiter (5 ms) holds output_peak_dbfs instead of a smaller
                                            # gain: with output_loudness the gain is no longer capped by the largest sample, without it the pre-gain is 1.
                                            # "true" limits a 4x oversampled estimate of the peak between the samples.  vv_pcm_limit on the HIP engine,
                                            # audio_processor.limit_peaks on injected sessions; synthesize_stream honours it (without output_loudness)
    output_pitch: Optional[float] = None    # pitch shift in semitones, -12 ... 12: a WSOLA time stretch of the joined signal, then a rate
                                            # conversion, before the loudness step.  The formants move with the pitch.  vv_pcm_stretch on the HIP
                                            # engine, audio_processor.shift_prosody on injected sessions.  Not available in synthesize_stream
    output_tempo: Optional[float] = None    # tempo, 0.5 ... 2.0 times the speed, by the same stretch: the synthesis itself is untouched (``speed``
                                            # asks the model for another duration instead)
    output_formants: str = "shift"          # "shift" | "keep" (DESIGN §8 N18): what output_pitch does to the spectral envelope.  "shift" = it moves with
                                            # the pitch (N14 as ever); "keep" = an LPC envelope correction behind the rate conversion puts the envelope of
                                            # the joined signal back, the harmonics stay where the pitch put them.  Acts only where the pitch ratio is not
                                            # 1.  vv_pcm_formant on the HIP engine, audio_processor.keep_formants on injected sessions
    output_denoise: Optional[float] = None  # strength of the vocoder-bias denoiser, 0 < s <= 16: s times a stationary magnitude profile is
                                            # taken off the STFT magnitudes of the joined signal (clamped at zero, phases kept), before pitch and tempo.
                                            # vv_pcm_denoise on the HIP engine, audio_processor.denoise_pcm on the host.  Not available in synthesize_stream
    output_denoise_bias: Optional[Sequence[float]] = None      # the profile: 513 non-negative magnitudes (bins 0 ... 512 of a 1024-point Hann frame of
                                            # int16 samples).  None = the model's own: what its decoder emits for an empty mel (HipSynth.vocoder_bias),
                                            # which needs the HIP engine
    output_watermark_key: Optional[int] = None      # the key of the audio watermark, 0 ... 2^64 - 1; None = no watermark.  With a key
                                            # every utterance carries a 16-bit payload as a multiplicative spread-spectrum mark, embedded behind pitch and
                                            # tempo and before the loudness step; TTSEngine.detect_watermark reads it back.  vv_pcm_watermark on the HIP
                                            # engine, audio_processor.watermark_embed on the host.  Not available in synthesize_stream
    output_watermark_payload: int = 0       # the payload, 0 ... 65535 (a request id); a request may bring its own (submit(watermark_payload=))
    output_watermark_strength: float = 0.2  # the gain step a of the mark, 0 < a <= 0.5: a band cell is scaled by 1 + a or 1 - a

    def __post_init__(self):
        if not 0.1 <= self.speed <= 5.0:
            raise ValueError("Speed must be between 0.1 and 5.0")
        if not 1 <= self.nfe_step <= 100:
            raise ValueError("NFE step must be between 1 and 100")
        if self.acoustic_dtype not in ("bf16", "fp32"):
            raise ValueError("acoustic_dtype must be 'bf16' or 'fp32'")
        from ..model_spec import ODE_METHODS, ODE_MULTISTEP
        if self.ode_method not in ODE_METHODS and self.ode_method not in ODE_MULTISTEP:
            raise ValueError(f"ode_method must be one of {sorted(ODE_METHODS) + sorted(ODE_MULTISTEP)}")
        self.ode_report = bool(self.ode_report)
        if self.ode_report and self.ode_method not in ODE_MULTISTEP:
            raise ValueError(f"ode_report needs a multistep ode_method ({sorted(ODE_MULTISTEP)}): it reports the difference of consecutive slopes")
        if self.cfg_strength is not None:
            self.cfg_strength = float(self.cfg_strength)
            if self.cfg_strength != self.cfg_strength or abs(self.cfg_strength) == float("inf"):
                raise ValueError("cfg_strength must be a finite number or None")
        from ..model_spec import NOISE_SOURCES
        if self.noise_source not in NOISE_SOURCES:
            raise ValueError(f"noise_source must be one of {list(NOISE_SOURCES)}")
        if self.output_stage not in ("host", "device"):
            raise ValueError("output_stage must be 'host' or 'device'")
        from .audio_processor import OUTPUT_ENCODINGS
        if self.output_encoding not in OUTPUT_ENCODINGS:
            raise ValueError(f"output_encoding must be one of {list(OUTPUT_ENCODINGS)}")
        from .audio_processor import check_flac_lpc_order
        if check_flac_lpc_order(self.flac_lpc_order) and self.output_encoding != "flac":
            raise ValueError("flac_lpc_order above 0 needs output_encoding 'flac'")
        if self.output_sample_rate is not None:
            if isinstance(self.output_sample_rate, bool) or int(self.output_sample_rate) != self.output_sample_rate:
                raise ValueError("output_sample_rate must be an integer number of Hz or None")
            self.output_sample_rate = int(self.output_sample_rate)
            if not 4000 <= self.output_sample_rate <= 192000:
                raise ValueError("output_sample_rate must be between 4000 and 192000 Hz")
        from .audio_processor import check_loudness
        self.output_loudness, self.output_peak_dbfs = check_loudness(self.output_loudness, self.output_peak_dbfs)
        from .audio_processor import check_limiter
        check_limiter(self.output_limiter)
        from .audio_processor import check_prosody
        self.output_pitch, self.output_tempo = check_prosody(self.output_pitch, self.output_tempo)
        from .audio_processor import check_formants
        self.output_formants = check_formants(self.output_formants)
        from .audio_processor import check_denoise, check_denoise_bias
        self.output_denoise = check_denoise(self.output_denoise)
        bias = check_denoise_bias(self.output_denoise_bias)
        self.output_denoise_bias = None if bias is None else [float(v) for v in bias]      # a plain list: to_dict / JSON keep working
        from .audio_processor import check_watermark_key, check_watermark_payload, check_watermark_strength
        self.output_watermark_key = check_watermark_key(self.output_watermark_key)
        if self.output_watermark_payload is None:
            raise ValueError("the watermark payload must be an integer in 0 ... 65535")
        self.output_watermark_payload = check_watermark_payload(self.output_watermark_payload)
        self.output_watermark_strength = check_watermark_strength(self.output_watermark_strength)
        from ..model_spec import check_cfg_interval
        self.cfg_interval = check_cfg_interval(self.cfg_interval)      # (lo, hi) floats, 0 <= lo <= hi <= 1; a list (from_dict of JSON) becomes the tuple
        from ..model_spec import check_apg
        check_apg(self.apg_eta, self.apg_norm)                          # finite eta, finite norm > 0; both None (or eta 1) = plain CFG
        self.apg_eta = None if self.apg_eta is None else float(self.apg_eta)
        self.apg_norm = None if self.apg_norm is None else float(self.apg_norm)
        from ..model_spec import check_cfg_reuse
        self.cfg_reuse = check_cfg_reuse(self.cfg_reuse)               # an integer >= 1 or None; 1 = off
        self.cfg_reuse_report = bool(self.cfg_reuse_report)
        if (self.cfg_reuse or 1) > 1 and check_apg(self.apg_eta, self.apg_norm) is not None:
            raise ValueError("cfg_reuse > 1 cannot be combined with apg_eta / apg_norm (projected guidance needs both predictions at every evaluation)")
        if self.cfg_reuse_report and not (self.cfg_reuse or 1) > 1:
            raise ValueError("cfg_reuse_report needs cfg_reuse > 1: it reports the drift of the reused guidance difference")
        from ..model_spec import check_block_cache
        self.block_cache = check_block_cache(self.block_cache, 1 << 30)     # three integers; a list (from_dict of JSON) becomes the tuple
        self.block_cache_interval = check_cfg_interval(self.block_cache_interval)
        self.block_cache_report = bool(self.block_cache_report)
        if self.block_cache is not None:
            if self.cfg_interval is not None or (self.cfg_reuse or 1) > 1 or check_apg(self.apg_eta, self.apg_norm) is not None:
                raise ValueError("block_cache cannot be combined with cfg_interval, cfg_reuse > 1 or apg_eta / apg_norm (a guided subset moves the "
                                 "unconditional rows between evaluations, which the stored rows do not follow)")
        elif self.block_cache_report or self.block_cache_interval is not None:
            raise ValueError("block_cache_report and block_cache_interval need block_cache")
        from ..model_spec import check_cfg_norm, check_cfg_norm_combination, check_cfg_zero_init
        if not isinstance(self.cfg_zero_star, bool):
            raise ValueError("cfg_zero_star must be a bool")
        check_cfg_norm(self.cfg_zero_star, self.cfg_rescale)             # phi a finite number in (0, 1], or None
        self.cfg_rescale = None if self.cfg_rescale is None else float(self.cfg_rescale)
        check_cfg_norm_combination(self.cfg_zero_star, self.cfg_rescale, self.apg_eta, self.apg_norm, self.cfg_reuse, self.block_cache)
        self.cfg_zero_init = check_cfg_zero_init(self.cfg_zero_init, self.nfe_step)
        self.cfg_norm_report = bool(self.cfg_norm_report)
        if self.cfg_norm_report and check_cfg_norm(self.cfg_zero_star, self.cfg_rescale) is None:
            raise ValueError("cfg_norm_report needs cfg_zero_star or cfg_rescale: it reports their coefficients")
        self.validate_paths()

    @property
    def model_path(self) -> str:
        return str(Path(self.model_cache_dir).expanduser() / self.model_filename)

    def ensure_model_downloaded(self) -> str:
        """Return the path of the cached model pack (the reference would fetch it; we cannot)."""
        path = Path(self.model_path)
        path.parent.mkdir(parents=True, exist_ok=True)
        if path.exists():
            return str(path)
        if self.synthetic_model or os.environ.get("VIETVOICE_TTS_SYNTHETIC") == "1":
            from ..model_pack import write_synthetic_pack
            logger.info("no cached model at %s: writing a seeded synthetic model pack (%s)", path, self.model_spec)
            write_synthetic_pack(str(path), self.model_spec, seed=self.random_seed)
            return str(path)
        raise RuntimeError(
            f"Failed to download model from {self.model_url}: no network access in this build; place the model pack at "
            f"{path} or set synthetic_model=True / VIETVOICE_TTS_SYNTHETIC=1")

    def validate_paths(self):
        try:
            self.ensure_model_downloaded()
        except Exception as e:
            raise RuntimeError(f"Model validation failed: {e}")

    def validate_with_reference_audio(self, reference_audio_path: str) -> bool:
        """max_chunk_duration must leave room for the clip + 1 s margin + min_target_duration
        (reference model_config.py:114-141)."""
        try:
            from .audio_processor import AudioProcessor
            ref_duration = AudioProcessor.probe_duration(reference_audio_path)
            needed = ref_duration + 1.0 + self.min_target_duration
            if self.max_chunk_duration < needed:
                logger.error("Configuration Error: reference audio %.1fs needs max_chunk_duration > %.1fs (is %.1fs)",
                             ref_duration, needed, self.max_chunk_duration)
                return False
            logger.info("Configuration valid: reference audio %.1fs, %.1fs available per chunk", ref_duration,
                        self.max_chunk_duration - ref_duration - 1.0)
            return True
        except Exception as e:      # same contract as the reference: never raises, returns False
            logger.error("Error validating reference audio: %s", e)
            return False

    @classmethod
    def from_dict(cls, config_dict: dict) -> "ModelConfig":
        return cls(**config_dict)

    def to_dict(self) -> dict:
        return {f.name: getattr(self, f.name) for f in fields(self)}


TTSConfig = ModelConfig   # backward-compatibility alias, as in the reference
