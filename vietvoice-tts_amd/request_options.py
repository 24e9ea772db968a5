"""What one request may ask for beside its text, speed and voice: one record from ``BatchingFrontend.submit`` to the stage that consumes
each value.  A new per-request option is a field here, its check in ``checked``, and its use in that one stage.  The
record of N21 -- eleven fields, ``cfg_reuse`` the last -- is what every request without a watermark payload carries, unchanged; a request
with one carries ``MarkedRequestOptions``, the same record with that field behind the eleven; a request with ``cfg_zero_star`` or
``cfg_rescale`` (N24) carries ``NormedRequestOptions``, with those two behind the payload (the tests of the eleven-field record pin its
length, so the new fields cannot live in it)."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import List, Optional, Tuple


@dataclass(frozen=True)
class RequestOptions:
    """None = the engine's value (``resolved``).  ``watermark_payload`` (N22) reads None here; MarkedRequestOptions carries one."""
    cfg_strength: Optional[float] = None                   # the acoustic stage, per chunk (N7)
    cfg_interval: Optional[Tuple[float, float]] = None     # (N8)
    apg_eta: Optional[float] = None                        # (N11)
    apg_norm: Optional[float] = None
    loudness: Optional[float] = None                       # the output stage, per request (N12)
    limiter: Optional[str] = None                          # (N13)
    pitch: Optional[float] = None                          # (N14)
    tempo: Optional[float] = None
    formants: Optional[str] = None                         # (N18)
    denoise: Optional[float] = None                        # (N19)
    cfg_reuse: Optional[int] = None                        # the acoustic stage, per chunk (N21)
    watermark_payload = None                               # no field: only MarkedRequestOptions has a payload (N22)
    cfg_zero_star = None                                   # no fields: only NormedRequestOptions has them (N24)
    cfg_rescale = None

    @classmethod
    def checked(cls, cfg_strength=None, cfg_interval=None, apg_eta=None, apg_norm=None, loudness=None, limiter=None, pitch=None, tempo=None,
                formants=None, denoise=None, cfg_reuse=None, watermark_payload=None, cfg_zero_star=None, cfg_rescale=None) -> "RequestOptions":
        """The validated, normalised record; ValueError in the words of the option's own check, the first in this order."""
        from .core.audio_processor import check_denoise, check_formants, check_limiter, check_loudness, check_prosody, check_watermark_payload
        from .model_spec import check_apg, check_cfg_interval, check_cfg_norm, check_cfg_reuse
        loudness, _pk = check_loudness(loudness)
        check_limiter(limiter)
        pitch, tempo = check_prosody(pitch, tempo)
        formants = None if formants is None else check_formants(formants)
        denoise = check_denoise(denoise)
        cfg_interval = check_cfg_interval(cfg_interval)
        check_apg(apg_eta, apg_norm)
        apg_eta, apg_norm = (None if v is None else float(v) for v in (apg_eta, apg_norm))
        if cfg_strength is not None:
            cfg_strength = float(cfg_strength)
            if cfg_strength != cfg_strength or abs(cfg_strength) == float("inf"):
                raise ValueError("cfg_strength must be a finite number or None")
        cfg_reuse = check_cfg_reuse(cfg_reuse)
        watermark_payload = check_watermark_payload(watermark_payload)
        check_cfg_norm(cfg_zero_star, cfg_rescale)
        cfg_rescale = None if cfg_rescale is None else float(cfg_rescale)
        eleven = (cfg_strength, cfg_interval, apg_eta, apg_norm, loudness, limiter, pitch, tempo, formants, denoise, cfg_reuse)
        return _record(eleven, watermark_payload, cfg_zero_star, cfg_rescale)

    def resolved(self, config) -> "RequestOptions":
        """Every None replaced by the engine's value: the one place that says "own value, else the engine's".  The watermark payload is the
        engine's only where the engine has a key (the result is then a MarkedRequestOptions); a payload of its own on an engine without
        a key is refused."""
        keyed = getattr(config, "output_watermark_key", None) is not None
        payload = self.watermark_payload
        if payload is not None and not keyed:
            raise ValueError("watermark_payload needs an engine with output_watermark_key")
        if payload is None and keyed:
            payload = getattr(config, "output_watermark_payload", 0)
        mine = RequestOptions(config.cfg_strength, config.cfg_interval, config.apg_eta, config.apg_norm, config.output_loudness,
                              config.output_limiter, config.output_pitch, config.output_tempo, config.output_formants, config.output_denoise,
                              getattr(config, "cfg_reuse", None))
        full = replace(mine, **{name: v for name, v in vars(self).items() if v is not None and name in vars(mine)})
        star = self.cfg_zero_star if self.cfg_zero_star is not None else (True if getattr(config, "cfg_zero_star", False) else None)
        rescale = self.cfg_rescale if self.cfg_rescale is not None else getattr(config, "cfg_rescale", None)
        return _record(tuple(vars(full).values()), payload, star, rescale)

    def wants_output_stage(self) -> bool:
        """Some step behind the join is asked for: what ``TTSEngine._device_output`` asks of the requests."""
        return any(v is not None for v in (self.loudness, self.limiter, self.pitch, self.tempo, self.denoise, self.watermark_payload))


@dataclass(frozen=True)
class MarkedRequestOptions(RequestOptions):
    """A request's options with a watermark payload (N22): 0 ... 65535, embedded under the engine's ``output_watermark_key``."""
    watermark_payload: Optional[int] = None


@dataclass(frozen=True)
class NormedRequestOptions(MarkedRequestOptions):
    """A request's options with CFG-Zero*'s optimised scale and / or a guidance rescale (N24; model_spec.check_cfg_norm): ``cfg_zero_star``
    True / False (False = off whatever the engine says), ``cfg_rescale`` phi in (0, 1].  ``watermark_payload`` may be None here."""
    cfg_zero_star: Optional[bool] = None
    cfg_rescale: Optional[float] = None


def _record(eleven, watermark_payload, cfg_zero_star, cfg_rescale) -> RequestOptions:
    """The smallest of the three records that holds the values."""
    if cfg_zero_star is not None or cfg_rescale is not None:
        return NormedRequestOptions(*eleven, watermark_payload, cfg_zero_star, cfg_rescale)
    return RequestOptions(*eleven) if watermark_payload is None else MarkedRequestOptions(*eleven, watermark_payload)


def column(options: List[RequestOptions], name: str) -> Optional[list]:
    """One field of every entry, or None when no entry has it."""
    vals = [getattr(o, name) for o in options]
    return None if all(v is None for v in vals) else vals
