"""Request-batching front end: coalesce concurrent ``synthesize`` calls into GPU batches.

The reference REST layer pushes each request onto a worker thread against ONE engine that is not thread safe and
mutates ``engine.config.speed`` around the call (api/tts_engine.py:64-91).  Here every request carries its own speed,
all chunks of all waiting requests are flattened into ragged GPU batches (different reference clips per item are
fine: per-item lengths live on the device), and each request gets its own cross-faded PCM back through a Future.
Noise is drawn from a per-request generator seeded with (config.random_seed, request serial) -- or, with ``noise_source="device"``, in
HBM from the Philox streams (config.random_seed, request serial, chunk) of model_spec.noise_keys -- and every kernel of the
path is row- or sequence-local with one arithmetic whatever the launch size (round 4: the split-K tail is off, the two
GEMM kernels share their epilogue arithmetic), so a request's audio does not depend on which other requests happened to
share its batch -- bit for bit (tests/test_engine_gpu.py::test_batching_frontend_batch_composition_invariance*).

Round 4: the loop is a three-stage pipeline instead of collect -> GPU -> cross-fade -> collect on one thread:

  preparer   collects requests, runs the host side of each (``select_sample``, ``_prepare_inputs``: text cleaning, chunk plan,
             voice-bank lookup; the per-request noise draw) and hands a prepared batch to the GPU stage.  While the GPU stage is
             busy it KEEPS COLLECTING into the waiting batch (up to ``max_requests``), so the batch that runs next holds
             everything that arrived during the previous one: under load the collect window is the GPU time of the batch in
             front, not ``max_wait_ms``.
  gpu        one ragged batch after the other through ``TTSEngine._synthesize_device`` (serialised by the engine lock).
  finisher   per-request cross-fade (host numpy, audio_processor.py:122-192; with the device output stage ONE finish_output call joins
             every request of the batch in HBM) and Future completion, off the GPU stage's path.

``overlap=False`` keeps the three stages on one thread in the old order (the A/B baseline and the equality test).
"""
from __future__ import annotations

import queue
import threading
import time
from concurrent.futures import Future
from typing import NamedTuple, Optional, Tuple

import numpy as np

from .request_options import RequestOptions


class _Request(NamedTuple):
    """What travels through the request queue."""
    serial: int
    text: str
    speed: Optional[float]
    voice: dict
    fut: Future
    options: RequestOptions


class _Batch:
    __slots__ = ("reqs", "flat", "blocks", "keys", "t0")

    def __init__(self):
        self.reqs = []                # per REQUEST: (its Future, the number of its chunks, its RequestOptions)
        self.flat, self.blocks, self.keys = [], [], []      # per CHUNK, the requests' one after another: inputs, and noise blocks or key rows
        self.t0 = time.time()


class BatchingFrontend:
    def __init__(self, engine, max_wait_ms: float = 5.0, max_requests: int = 16, overlap: bool = True):
        self.engine = engine
        self.max_wait = max_wait_ms / 1e3
        self.max_requests = max_requests
        self.overlap = bool(overlap)
        self._q: "queue.Queue" = queue.Queue()
        self._ready: "queue.Queue" = queue.Queue(maxsize=1)      # prepared batches waiting for the GPU stage
        self._done: "queue.Queue" = queue.Queue()                # synthesised batches waiting for their cross-fades
        self._serial = 0
        self._serial_lock = threading.Lock()
        self._closed = False           # close() has been called: submit() refuses (set under _serial_lock)
        self._stage_down = False       # the collecting stage has ended (normally or not): nothing will take a request off the queue any more
        self._closing = False          # the close() sentinel has been taken off the request queue
        self.batches_run = 0
        self.requests_done = 0
        self.chunks_run = 0
        self.frames_run = 0
        self.gpu_busy_s = 0.0
        if self.overlap:
            self._threads = [threading.Thread(target=self._prep_loop, name="vvtts-batcher-prep", daemon=True),
                             threading.Thread(target=self._gpu_loop, name="vvtts-batcher-gpu", daemon=True),
                             threading.Thread(target=self._finish_loop, name="vvtts-batcher-finish", daemon=True)]
        else:
            self._threads = [threading.Thread(target=self._serial_loop, name="vvtts-batcher", daemon=True)]
        for t in self._threads:
            t.start()

    def submit(self, text: str, speed: Optional[float] = None, serial: Optional[int] = None, cfg_strength: Optional[float] = None,
               cfg_interval: Optional[Tuple[float, float]] = None, apg_eta: Optional[float] = None, apg_norm: Optional[float] = None,
               loudness: Optional[float] = None, limiter: Optional[str] = None, pitch: Optional[float] = None, tempo: Optional[float] = None,
               formants: Optional[str] = None, denoise: Optional[float] = None, cfg_reuse: Optional[int] = None, watermark_payload: Optional[int] = None,
               cfg_zero_star: Optional[bool] = None, cfg_rescale: Optional[float] = None, **voice) -> Future:
        """voice: gender / group / area / emotion / sample_iteration / reference_audio / reference_text.
        ``serial`` fixes the request's noise stream (default: arrival counter).  ``cfg_strength``: this request's guidance strength
        (None = the engine's), carried per item into the batch -- the audio does not depend on the strengths of its batch neighbours.
        ``cfg_interval``: this request's guidance interval (lo, hi), 0 <= lo <= hi <= 1 (None = the engine's), per item in the same way.
        ``apg_eta`` / ``apg_norm``: this request's projected guidance (model_spec.check_apg; None = the engine's value), per item as well:
        plain and projected requests share one batch.  ``loudness``: this request's programme loudness in LUFS (-60 ... -5, DESIGN §8 N12;
        None = the engine's ``output_loudness``), measured and applied to this request alone in the batch's one finish_output call.
        ``limiter``: this request's limiter, "sample" or "true" (None = the engine's ``output_limiter``), carried the same way.
        ``pitch`` (semitones, -12 ... 12) / ``tempo`` (0.5 ... 2.0): this request's prosody (None = the engine's
        ``output_pitch`` / ``output_tempo``), applied to this request alone; its batch neighbours are copied untouched.
        ``formants``: "shift" or "keep" (None = the engine's ``output_formants``): what this request's pitch does to its
        spectral envelope, carried the same way.
        ``denoise``: this request's denoiser strength, 0 < s <= 16 (None = the engine's ``output_denoise``), applied to this
        request alone, against the engine's bias profile.
        ``cfg_reuse``: this request's guidance reuse k (None = the engine's ``cfg_reuse``, 1 = off): its unconditional branch
        runs at every k-th guided evaluation only, per item beside the interval and the strength in one ragged batch.  Together with an
        ``apg_eta`` / ``apg_norm`` that is not off (its own or the engine's) the request fails with a ValueError.
        ``watermark_payload``: this request's watermark payload, 0 ... 65535 (None = the engine's
        ``output_watermark_payload``), embedded in this request alone under the engine's ``output_watermark_key``; on an engine without a
        key the request fails with a ValueError.
        On an engine with ``block_cache`` every batch caches blocks; a request that brings a ``cfg_interval``, a ``cfg_reuse``
        above 1 or projected guidance fails with a ValueError.
        ``cfg_zero_star`` / ``cfg_rescale``: this request's CFG-Zero* optimised scale (True / False) and guidance rescale phi, 0 < phi <= 1
        (None = the engine's ``cfg_zero_star`` / ``cfg_rescale``), per item beside the strength and the interval in one ragged
        batch.  Together with projected guidance, with a ``cfg_reuse`` above 1 or on an engine with ``block_cache`` the request fails with a
        ValueError (zero-init, ``cfg_zero_init``, is the engine's alone, as ``ode_method`` is)."""
        fut: Future = Future()
        try:
            options = RequestOptions.checked(cfg_strength=cfg_strength, cfg_interval=cfg_interval, apg_eta=apg_eta, apg_norm=apg_norm,
                                             loudness=loudness, limiter=limiter, pitch=pitch, tempo=tempo, formants=formants, denoise=denoise,
                                             cfg_reuse=cfg_reuse, watermark_payload=watermark_payload, cfg_zero_star=cfg_zero_star,
                                             cfg_rescale=cfg_rescale)
            config = getattr(self.engine, "config", None)
            full = options if config is None else options.resolved(config)
            from .model_spec import check_apg, check_cfg_norm_combination
            check_cfg_norm_combination(full.cfg_zero_star, full.cfg_rescale, full.apg_eta, full.apg_norm, full.cfg_reuse,
                                       getattr(config, "block_cache", None))
            if (full.cfg_reuse or 1) > 1 and check_apg(full.apg_eta, full.apg_norm) is not None:
                raise ValueError("cfg_reuse > 1 cannot be combined with apg_eta / apg_norm (projected guidance needs both predictions at every evaluation)")
            if getattr(config, "block_cache", None) is not None and (full.cfg_interval is not None or (full.cfg_reuse or 1) > 1
                                                                     or check_apg(full.apg_eta, full.apg_norm) is not None):
                raise ValueError("this engine caches blocks (block_cache): a request cannot bring a cfg_interval, cfg_reuse > 1 or apg_eta / apg_norm "
                                 "(a guided subset moves the unconditional rows between evaluations, which the stored rows do not follow)")
        except ValueError as e:
            fut.set_exception(e)
            return fut
        with self._serial_lock:           # close() raises `_closed` under the same lock: a request is either queued in front of the
            if self._closed or self._stage_down:      # sentinel (and served) or refused here -- never orphaned behind it
                fut.set_exception(RuntimeError("Speech synthesis failed: the batching front end is closed"))
                return fut
            if serial is None:
                serial = self._serial
            self._serial = max(self._serial, serial) + 1
            self._q.put(_Request(serial, text, speed, voice, fut, options))
        return fut

    def synthesize(self, text: str, speed: Optional[float] = None, **voice) -> Tuple[np.ndarray, float]:
        return self.submit(text, speed, **voice).result()

    def close(self):
        """Drain and stop: requests submitted before the call are still served (the sentinel queues up behind them); a request that
        could not be (a stage died, the join timed out) gets an exception instead of a Future that never completes."""
        with self._serial_lock:
            if self._closed:
                return
            self._closed = True
            self._q.put(None)
        for t in self._threads:
            t.join(timeout=120)
        while True:
            try:
                req = self._q.get_nowait()
            except queue.Empty:
                break
            if req is not None and not req.fut.done():
                req.fut.set_exception(RuntimeError("Speech synthesis failed: the batching front end is closed"))

    def stats(self) -> dict:
        b = max(self.batches_run, 1)
        return {"batches": self.batches_run, "requests": self.requests_done, "requests_per_batch": self.requests_done / b,
                "chunks_per_batch": self.chunks_run / b, "frames_per_batch": self.frames_run / b, "gpu_busy_s": self.gpu_busy_s}

    # ------------------------------------------------------------------ stage 1: collect + host preparation
    def _prepare_one(self, req: _Request, batch: _Batch) -> None:
        import torch
        eng = self.engine
        voice, fut = req.voice, req.fut
        try:
            ref_audio, ref_text = eng.model_session_manager.select_sample(
                voice.get("gender"), voice.get("group"), voice.get("area"), voice.get("emotion"), voice.get("sample_iteration"),
                voice.get("reference_audio"), voice.get("reference_text"))
        except Exception as e:          # propagate unwrapped, as TTSEngine.synthesize does (tts_engine.py:217)
            fut.set_exception(e)
            return
        try:
            inputs = eng._prepare_inputs(ref_audio, ref_text, req.text, speed=req.speed)
        except Exception as e:
            fut.set_exception(RuntimeError(f"Speech synthesis failed: {e}"))
            return
        try:
            blocks, keys = [], []
            if eng._device_noise():         # N9: nothing is drawn here -- the request's serial names its Philox streams, chunk by chunk
                from .model_spec import noise_keys
                keys = list(noise_keys(eng.config.random_seed, req.serial, len(inputs)))
            else:
                n_mel = eng.model_session_manager.spec.n_mel
                gen = torch.Generator().manual_seed(eng.config.random_seed * 1000003 + req.serial)
                blocks = [torch.randn((int(i[2][0]), n_mel), generator=gen, dtype=torch.float32) for i in inputs]
        except Exception as e:          # noqa: BLE001  (nothing of this request has entered the batch yet)
            fut.set_exception(RuntimeError(f"Speech synthesis failed: {e}"))
            return
        batch.reqs.append((fut, len(inputs), req.options))
        batch.flat.extend(inputs)
        batch.blocks.extend(blocks)
        batch.keys.extend(keys)

    def _collect(self) -> Optional[_Batch]:
        """Block for the first request, then take what arrives within ``max_wait`` -- and whatever is ALREADY queued when the window
        closes (the window bounds the wait for arrivals, not the time spent on requests that are there) -- up to ``max_requests``;
        the host preparation of the collected requests follows.  None = the close() sentinel arrived with nothing collected."""
        if self._closing:
            return None
        first = self._q.get()
        if first is None:
            self._closing = True
            return None
        reqs = [first]
        deadline = time.monotonic() + self.max_wait
        while len(reqs) < self.max_requests:
            left = deadline - time.monotonic()
            try:
                nxt = self._q.get(timeout=left) if left > 0 else self._q.get_nowait()
            except queue.Empty:
                break
            if nxt is None:
                self._closing = True
                break
            reqs.append(nxt)
        batch = _Batch()
        for k, r in enumerate(reqs):
            try:
                self._prepare_one(r, batch)
            except BaseException as e:    # noqa: BLE001  (_prepare_one reports its own failures; this is the last line of defence)
                if not r.fut.done():
                    r.fut.set_exception(RuntimeError(f"Speech synthesis failed: {e!r}"))
                if not isinstance(e, Exception):          # the stage is going down: nothing taken off the queue may be left pending
                    for later in reqs[k + 1:]:
                        later.fut.set_exception(RuntimeError(f"Speech synthesis failed: {e!r}"))
                    self._fail(batch, e)
                    raise
        return batch

    @staticmethod
    def _fail(batch: Optional[_Batch], err) -> None:
        if batch is not None:
            for fut, _n, _o in batch.reqs:
                if not fut.done():
                    fut.set_exception(RuntimeError(f"Speech synthesis failed: {err}"))

    def _prep_loop(self):
        self._in_hand = None
        try:
            self._prep_body()
        except BaseException as e:        # noqa: BLE001  (the batch being handed over dies with the stage, loudly)
            self._closing = True
            self._fail(self._in_hand, e)
            self._drain_requests(e)
            if not isinstance(e, Exception):
                raise
        finally:
            with self._serial_lock:        # from here on submit() refuses; whatever raced in before is failed, not stranded
                self._stage_down = True
            self._drain_requests("the batching front end has stopped")
            self._ready.put(None)          # whatever happened here, the stages behind must see the end of the stream

    def _prep_body(self):
        while True:
            try:
                batch = self._collect()
            except Exception as e:        # noqa: BLE001  (an unexpected failure while collecting: stop taking requests)
                self._closing = True
                self._drain_requests(e)
                return
            if batch is None:
                break
            self._in_hand = batch
            # hand over; while the GPU stage still has a batch waiting in front, keep filling this one (a collected batch is always
            # delivered, also when close() arrives meanwhile)
            while batch.flat:
                try:
                    self._ready.put(batch, timeout=0.002)
                    self._in_hand = None
                    break
                except queue.Full:
                    pass
                if len(batch.reqs) < self.max_requests and not self._closing:
                    try:
                        nxt = self._q.get(timeout=0.002)
                    except queue.Empty:
                        continue
                    if nxt is None:
                        self._closing = True
                    else:
                        self._prepare_one(nxt, batch)

    def _drain_requests(self, err) -> None:
        while True:
            try:
                req = self._q.get_nowait()
            except queue.Empty:
                return
            if req is not None and not req.fut.done():
                req.fut.set_exception(RuntimeError(f"Speech synthesis failed: {err}"))

    # ------------------------------------------------------------------ stage 2: the GPU
    def _run_batch(self, batch: _Batch):
        eng = self.engine
        t0 = time.perf_counter()
        with eng._lock:
            if eng.model_session_manager.engine is not None:
                # N10: a request's own output option takes the device stage too: the chunks stay in HBM, _finish joins the whole batch in one call
                dev_out = eng._device_output([o for _f, _n, o in batch.reqs])
                noise = {"noise_keys": np.stack(batch.keys)} if batch.keys else {"noise_blocks": batch.blocks}
                waves = eng._synthesize_device(batch.flat, options=[o for _f, n, o in batch.reqs for _chunk in range(n)], device_out=dev_out, **noise)
            else:
                waves = eng._synthesize_sessions(batch.flat)      # CPU plumbing tests: the oracle sessions draw their own noise
        self.gpu_busy_s += time.perf_counter() - t0
        self.batches_run += 1
        self.chunks_run += len(batch.flat)
        self.frames_run += sum(int(i[2][0]) for i in batch.flat)
        return waves

    def _gpu_loop(self):
        try:
            while True:
                batch = self._ready.get()
                if batch is None:
                    break
                try:
                    self._done.put((batch, self._run_batch(batch), None))
                except BaseException as e:        # noqa: BLE001
                    self._done.put((batch, None, e))
                    if not isinstance(e, Exception):
                        raise
        finally:
            self._done.put(None)

    # ------------------------------------------------------------------ stage 3: cross-fade + completion
    def _finish(self, batch: _Batch, waves, err) -> None:
        eng = self.engine
        if err is not None:
            self._fail(batch, err)
            return
        if isinstance(waves, tuple):          # device output stage: (device PCM, spans) -- one finish_output call for the whole batch
            try:
                finals = eng._finish_device(waves, [n for _f, n, _o in batch.reqs], [o for _f, _n, o in batch.reqs])
            except Exception as e:        # noqa: BLE001
                self._fail(batch, e)
                return
            for (fut, _n, _o), final in zip(batch.reqs, finals):
                fut.set_result((final, time.time() - batch.t0))
                self.requests_done += 1
            return
        pos = 0
        for fut, n, options in batch.reqs:
            try:
                fut.set_result((eng._finish_host(waves[pos: pos + n], options), time.time() - batch.t0))
            except Exception as e:        # noqa: BLE001
                fut.set_exception(RuntimeError(f"Speech synthesis failed: {e}"))
            pos += n
            self.requests_done += 1

    def _finish_loop(self):
        while True:
            item = self._done.get()
            if item is None:
                break
            try:
                self._finish(*item)
            except Exception as e:        # noqa: BLE001  (never leave a Future of the batch in hand pending)
                self._fail(item[0], e)

    # ------------------------------------------------------------------ overlap=False: the three stages in order on one thread
    def _serial_loop(self):
        batch = None
        try:
            while True:
                batch = self._collect()
                if batch is None:
                    break
                if not batch.flat:
                    continue
                try:
                    waves, err = self._run_batch(batch), None
                except Exception as e:    # noqa: BLE001
                    waves, err = None, e
                self._finish(batch, waves, err)
        except BaseException as e:        # noqa: BLE001  (same promise as the pipelined stages: no Future left pending)
            self._fail(batch, e)
            self._drain_requests(e)
            if not isinstance(e, Exception):
                raise
        finally:
            with self._serial_lock:
                self._stage_down = True
            self._drain_requests("the batching front end has stopped")
