"""Engine: the batched recv → process → send loop.

Reference behavior being reproduced (/root/reference/src/service/features/
engine.py:73-342): a daemon thread listens on ``engine_addr``, polls with a
recv timeout (100 ms default), hands frames to the processor, skips
``None`` results (filtered messages, engine.py:238-240), broadcasts results
to every ``out_addr`` socket or — when no outputs are configured — replies
on the input pair socket (request/reply compatibility, engine.py:248-264).
Sends are non-blocking with ``engine_retry_count`` retries at 10 ms and
drop-with-counter on failure (engine.py:281-301). Output sockets dial
non-blocking with background reconnect (engine.py:173-175). ``stop()``
joins the thread with a 2 s deadline and raises ``EngineException`` if it
fails to stop cleanly (engine.py:317-323); the thread is re-created on
restart (engine.py:185-191). Setup failure closes the input socket to
avoid leaks (engine.py:122-129).

MI355X-first departure: the loop is **batch-first** —
``recv_many`` drains up to ``engine_batch_size`` frames (bounded by
``engine_batch_linger_ms``) and calls ``processor.process_batch(frames)``
once, so a GPU component launches one kernel per batch instead of one
Python call per message. Per-frame semantics (ordering, None-skip,
per-output drop accounting) are preserved exactly.
"""
from __future__ import annotations

import logging
import os
import threading
import time
from typing import Any, Callable, List, NamedTuple, Optional, Protocol, runtime_checkable

from ..settings import ServiceSettings
from ..utils.metrics import ServiceMetrics
from .sockets import PackedBatch, PairSocketFactory, RecvTimeout, SocketClosed


class EngineException(Exception):
    pass


@runtime_checkable
class Processor(Protocol):
    """Processing contract (reference engine.py:61-69) + batched extension."""

    def process(self, data: bytes) -> Optional[bytes]: ...

    def process_batch(self, frames: List[bytes]) -> List[Optional[bytes]]: ...


def _count_lines(data: bytes) -> int:
    """One frame = one log line; embedded newlines add more (reference
    counts ``raw.count(b'\\n')`` — engine.py:213 — which is 0 for protobuf
    frames; we floor at 1 so lines/sec matches frames of protobuf traffic)."""
    n = data.count(b"\n")
    return n if n > 0 else 1


class _LoopStats:
    """DMX_ENGINE_STATS=1 window (perf triage): named timers summed over ~2 s
    of batches; a loop logs its own line when ``due``, then calls ``reset``."""

    def __init__(self, *timers: str) -> None:
        self.on = os.environ.get("DMX_ENGINE_STATS") == "1"
        self._names = timers
        self.reset(time.perf_counter())

    def reset(self, now: float) -> None:
        self.n = self.frames = 0  # batches, their frames
        self.t = dict.fromkeys(self._names, 0.0)
        self._last = now

    def add(self, timer: str, seconds: float) -> None:
        if self.on:
            self.t[timer] += seconds

    def batch(self, frames: int, proc_seconds: float) -> None:
        if self.on:
            self.n += 1
            self.frames += frames
            self.t["proc"] += proc_seconds

    def due(self, now: float) -> bool:
        return self.on and self.n > 0 and now - self._last > 2.0

    def ms(self, timer: str) -> float:
        return self.t[timer] * 1e3 / self.n  # mean per batch


class _PackedPlane(NamedTuple):
    """What ``Engine._probe_packed`` resolved for the packed loop."""

    process: Callable                # process_packed_frames
    submit: Optional[Callable]       # submit_/collect_packed_frames: both
    collect: Optional[Callable]      # or neither (then not pipelined)
    reply_conn: Callable             # socket.reply_conn, else its send
    has_pending: Callable            # socket.has_pending, else "no"


class _InFlight(NamedTuple):
    """A submitted, not yet collected batch. It holds the batch itself, so
    its replies use ITS routes whatever the listener received since."""

    token: Any
    batch: PackedBatch
    t_submit: float


class Engine:
    def __init__(
        self,
        settings: ServiceSettings,
        processor: Processor,
        socket_factory: Optional[PairSocketFactory] = None,
        logger: Optional[logging.Logger] = None,
        metrics: Optional[ServiceMetrics] = None,
        dist_ctx=None,
    ) -> None:
        self.settings = settings
        self.processor = processor
        #: settings-driven placement (core.py builds it from dist_mode):
        #: an object with .mode/.rank/.world/.src — selects the fanout /
        #: stage loops below instead of the socket loop
        self._dist_ctx = dist_ctx
        self._log = logger or logging.getLogger(__name__)
        self._factory = socket_factory or PairSocketFactory()
        self.metrics = metrics or ServiceMetrics(
            settings.component_type, settings.component_id or "unknown"
        )

        self._stop_event = threading.Event()
        self._thread: Optional[threading.Thread] = None
        self._running = False
        #: set by the packed loop for its _emit/_drain/_submit methods
        self._plane: Optional[_PackedPlane] = None
        self._stats: Optional[_LoopStats] = None

        # Bind the input socket now (reference engine.py:111-117); on any
        # failure during output setup, close the input to avoid leaks
        # (engine.py:122-129).
        self._pair_sock = self._factory.create(
            settings.engine_addr,
            logger=self._log,
            tls_config=settings.tls_input,
            buffer_size=settings.engine_buffer_size,
        )
        try:
            self._out_socks = self._setup_output_sockets()
        except Exception:
            self._pair_sock.close()
            raise

    # ------------------------------------------------------------------
    def _setup_output_sockets(self):
        socks = []
        for addr in self.settings.out_addr:
            kwargs = dict(
                logger=self._log,
                tls_config=self.settings.tls_output,
                buffer_size=self.settings.engine_buffer_size,
            )
            try:
                socks.append(self._factory.create_dialer(
                    addr, dial_timeout_s=self.settings.dial_timeout / 1000.0,
                    **kwargs,
                ))
            except TypeError:
                # injected test factories may not take dial_timeout_s
                socks.append(self._factory.create_dialer(addr, **kwargs))
        return socks

    @property
    def running(self) -> bool:
        return self._running and self._thread is not None and self._thread.is_alive()

    def start(self) -> None:
        if self.running:
            self._log.debug("engine already running")
            return
        # Thread is re-created on every start (reference engine.py:185-191).
        self._stop_event.clear()
        self._running = True
        self._thread = threading.Thread(
            target=self._run_loop, name="EngineLoop", daemon=True
        )
        self._thread.start()
        self.metrics.engine_starts_total.inc()
        self.metrics.engine_running.state("running")

    def stop(self) -> None:
        self._stop_event.set()
        self._running = False
        thread = self._thread
        if thread is not None and thread.is_alive():
            thread.join(timeout=2.0)
            if thread.is_alive():
                raise EngineException("Engine thread failed to stop cleanly")
        self.metrics.engine_running.state("stopped")

    def close(self) -> None:
        """Close all sockets (after stop)."""
        try:
            self._pair_sock.close()
        except Exception:  # noqa: BLE001
            pass
        for s in self._out_socks:
            try:
                s.close()
            except Exception:  # noqa: BLE001
                pass

    # ------------------------------------------------------------------
    def _run_loop(self) -> None:
        ctx = self._dist_ctx
        if ctx is not None and ctx.world > 1 and ctx.mode in ("fanout", "stage"):
            return self._run_dist_loop()
        if self.settings.engine_source_mode:
            return self._run_source_loop()
        if self.settings.engine_packed_mode:
            plane = self._probe_packed()
            if plane is not None:
                return self._run_packed_loop(plane)
        return self._run_socket_loop()

    # -- accounting every loop shares -----------------------------------
    def _count_read(self, n_bytes: int, n_lines: int,
                    batch_size: Optional[int] = None) -> None:
        """``batch_size`` feeds the batch-size histogram; the dist loops,
        which never observed it, pass none."""
        m = self.metrics
        m.data_read_bytes_total.inc(n_bytes)
        m.data_read_lines_total.inc(n_lines)
        if batch_size is not None:
            m.engine_batch_size.observe(batch_size)

    def _count_processed(self, n_bytes: int, n_lines: int, elapsed: float) -> None:
        m = self.metrics
        m.data_processed_bytes_total.inc(n_bytes)
        m.data_processed_lines_total.inc(n_lines)
        m.observe_batch(elapsed, n_lines)

    def _count_written(self, out: bytes, ok: bool, n_lines: int = 0) -> None:
        """One output written (``ok``) or dropped. It counts as
        ``_count_lines(out)`` lines unless the caller says how many:
        packed alerts and dist hops count 1 per output."""
        m = self.metrics
        n_lines = n_lines or _count_lines(out)
        if ok:
            m.data_written_bytes_total.inc(len(out))
            m.data_written_lines_total.inc(n_lines)
        else:
            m.data_dropped_bytes_total.inc(len(out))
            m.data_dropped_lines_total.inc(n_lines)

    def _run_socket_loop(self) -> None:
        """The plain batched frame loop (also the elastic-degradation
        target when a dist collective path loses a peer)."""
        s = self.settings
        m = self.metrics
        self._log.info(
            "engine loop started on %s (batch_size=%d linger=%.1fms outputs=%d)",
            s.engine_addr, s.engine_batch_size, s.engine_batch_linger_ms,
            len(self._out_socks),
        )
        sock = self._pair_sock
        # a socket without per-frame reply(idx) answers its last sender
        reply = getattr(sock, "reply", lambda idx, out: sock.send(out, block=False))
        stats = _LoopStats("recv", "proc", "total")
        t_end = time.perf_counter()
        while not self._stop_event.is_set():
            try:
                t_r0 = time.perf_counter()
                frames = self._pair_sock.recv_many(
                    s.engine_batch_size, s.engine_recv_timeout, s.engine_batch_linger_ms
                )
                stats.add("recv", time.perf_counter() - t_r0)
            except RecvTimeout:
                continue
            except SocketClosed:
                break
            except OSError as exc:
                if self._stop_event.is_set():
                    break
                self._log.error("recv error: %s", exc)
                continue
            # Skip empty frames (reference engine.py:207-209) — but keep
            # each surviving frame's ORIGINAL batch index: the listener
            # recorded its per-frame conns for the unfiltered recv_many
            # batch, so reply(i) must be given pre-filter indices or
            # multi-peer replies route to the wrong sender.
            orig_idx = [i for i, f in enumerate(frames) if f]
            if len(orig_idx) != len(frames):
                frames = [frames[i] for i in orig_idx]
            if not frames:
                continue

            read_bytes = sum(len(f) for f in frames)
            read_lines = sum(_count_lines(f) for f in frames)
            self._count_read(read_bytes, read_lines, len(frames))

            t0 = time.perf_counter()
            try:
                outs = self.processor.process_batch(frames)
            except Exception as exc:  # noqa: BLE001 - loop must survive (engine.py:233-236)
                m.processing_errors_total.inc(len(frames))
                self._log.error("processing error on batch of %d: %s", len(frames), exc)
                continue
            elapsed = time.perf_counter() - t0
            self._count_processed(read_bytes, read_lines, elapsed)

            for i, out in enumerate(outs):
                if out is None:
                    continue  # filtered (engine.py:238-240)
                if self._out_socks:
                    self._send_to_outputs(out)
                else:
                    # request/reply fallback mode (engine.py:248-264);
                    # replies route to EACH frame's sender (multi-peer)
                    self._count_written(out, reply(orig_idx[i], out))
            if stats.on:
                now = time.perf_counter()
                stats.batch(len(frames), elapsed)
                stats.add("total", now - t_end)
                t_end = now
                if stats.due(now):
                    tot = stats.t["total"]
                    self._log.info(
                        "[stats] %d batches (%.0f fr/batch): recv-wait %.1fms/b, "
                        "process %.1fms/b, other %.1fms/b, %.0f lines/s",
                        stats.n, stats.frames / stats.n,
                        stats.ms("recv"), stats.ms("proc"),
                        stats.ms("total") - stats.ms("recv") - stats.ms("proc"),
                        stats.frames / tot if tot > 0 else 0.0,
                    )
                    stats.reset(now)
        self._log.info("engine loop exited")

    # -- native packed data plane ----------------------------------------
    def _probe_packed(self) -> Optional[_PackedPlane]:
        """The packed plane needs a component with ``process_packed_frames``
        and a listener that can decode socket→tensor (plain fd or shm, with
        the C++ extension); else warn, and None selects the frame loop."""
        s, p, sock = self.settings, self.processor, self._pair_sock
        process = getattr(p, "process_packed_frames", None)
        supports = getattr(p, "supports_packed_frames", None)
        if process is None or (supports is not None and not supports()):
            self._log.warning(
                "engine_packed_mode: component has no process_packed_frames; "
                "using the frame loop"
            )
            return None
        enable = getattr(sock, "enable_packed", None)
        max_len = getattr(p, "packed_max_len", lambda: 256)()
        pin = getattr(p, "packed_pin_memory", lambda: False)()
        if enable is None or not enable(max_len, pin, s.engine_batch_size):
            self._log.warning(
                "engine_packed_mode: listener cannot enable the packed path "
                "(TLS/ws/inproc or extension missing); using the frame loop"
            )
            return None
        # pipelined mode: overlap batch N's async GPU work with batch
        # N+1's recv+decode (submit launches without syncing; collect
        # does the one readback). Falls back to the synchronous call
        # when the component lacks the split API.
        submit = getattr(p, "submit_packed_frames", None)
        collect = getattr(p, "collect_packed_frames", None)
        if submit is None or collect is None:
            submit = collect = None
        self._log.info(
            "engine PACKED loop started on %s (max_len=%d pin=%s pipelined=%s)",
            s.engine_addr, max_len, pin, submit is not None)
        return _PackedPlane(
            process, submit, collect,
            getattr(sock, "reply_conn", lambda conn, out: sock.send(out, block=False)),
            # a socket that cannot tell counts as idle: drain at once
            getattr(sock, "has_pending", lambda: False))

    def _run_packed_loop(self, plane: _PackedPlane) -> None:
        """Reader threads decode LogSchema frames straight into tensors
        (frame_reader.cpp read_batch_packed); the loop hands (lines, lens,
        ids) to the component with ZERO per-frame Python objects. At most
        one batch is in flight: it is drained before the next submit, on
        an idle or empty receive, and on exit."""
        s = self.settings
        self._plane = plane
        stats = self._stats = _LoopStats("recv", "proc", "submit", "drain")
        inflight: Optional[_InFlight] = None
        while not self._stop_event.is_set():
            try:
                t_r0 = time.perf_counter()
                batch = self._pair_sock.recv_packed(
                    s.engine_recv_timeout, s.engine_batch_size, s.engine_batch_linger_ms)
                stats.add("recv", time.perf_counter() - t_r0)
            except RecvTimeout:
                batch = None
            except SocketClosed:
                break
            except OSError as exc:
                if self._stop_event.is_set():
                    break
                self._log.error("recv error: %s", exc)
                continue
            B = int(batch.lines.shape[0]) if batch is not None else 0
            if B == 0:  # idle, or an empty batch: finish the in-flight one
                self._drain(inflight)
                inflight = None
                continue
            self._count_read(batch.nbytes, B, B)
            t0 = time.perf_counter()
            if plane.submit is None:
                self._process_packed(batch, t0)
            else:
                # collect batch N (the GPU overlapped our recv), launch N+1
                self._drain(inflight)
                inflight = self._submit(batch, t0)
                # sparse traffic: if nothing else is already queued,
                # finish this batch NOW instead of waiting out the recv
                # timeout (keeps single-frame round-trip latency low;
                # under load the queue is non-empty and pipelining holds)
                if not plane.has_pending():
                    self._drain(inflight)
                    inflight = None
            now = time.perf_counter() if stats.on else 0.0
            if stats.due(now):
                self._log.info(
                    "[packed-stats] %d batches (%.0f fr/b): recv-wait %.1fms/b "
                    "process %.1fms/b (submit %.1f drain %.1f)",
                    stats.n, stats.frames / stats.n, stats.ms("recv"),
                    stats.ms("proc"), stats.ms("submit"), stats.ms("drain"))
                stats.reset(now)
        self._drain(inflight)
        self._log.info("engine packed loop exited")

    def _packed_error(self, batch: PackedBatch, exc: Exception) -> None:
        """A component error costs its batch; the loop must survive."""
        B = int(batch.lines.shape[0])
        self.metrics.processing_errors_total.inc(B)
        self._log.error("processing error on packed batch of %d: %s", B, exc)

    def _process_packed(self, batch: PackedBatch, t0: float) -> None:
        """Synchronous branch: the component lacks submit/collect."""
        try:
            alerts = self._plane.process(batch.lines, batch.lens,
                                         batch.ids_blob, batch.ids_off)
        except Exception as exc:  # noqa: BLE001
            return self._packed_error(batch, exc)
        elapsed = time.perf_counter() - t0
        B = int(batch.lines.shape[0])
        self._count_processed(batch.nbytes, B, elapsed)
        self._emit(alerts, batch)
        self._stats.batch(B, elapsed)

    def _submit(self, batch: PackedBatch, t0: float) -> Optional[_InFlight]:
        """Launch ``batch`` without syncing; None when the component raised."""
        try:
            token = self._plane.submit(batch.lines, batch.lens,
                                       batch.ids_blob, batch.ids_off)
        except Exception as exc:  # noqa: BLE001
            return self._packed_error(batch, exc)
        self._stats.add("submit", time.perf_counter() - t0)
        return _InFlight(token, batch, t0)

    def _emit(self, alerts, batch: PackedBatch) -> None:
        """Send each (row, alert): to the outputs, or back to the row's
        sender as ``batch`` recorded it."""
        for idx, out in alerts:
            if self._out_socks:
                self._send_to_outputs(out)
            else:
                ok = self._plane.reply_conn(batch.conn_of(idx), out)
                self._count_written(out, ok, 1)

    def _drain(self, inflight: Optional[_InFlight]) -> None:
        """Collect a submitted batch and emit its alerts (no-op for None).
        The caller forgets ``inflight`` afterwards, also after an error."""
        if inflight is None:
            return
        batch = inflight.batch
        t_d0 = time.perf_counter()
        try:
            self._emit(self._plane.collect(inflight.token), batch)
        except Exception as exc:  # noqa: BLE001
            return self._packed_error(batch, exc)
        now = time.perf_counter()
        B = int(batch.lines.shape[0])
        self._count_processed(batch.nbytes, B, now - inflight.t_submit)
        self._stats.batch(B, now - inflight.t_submit)
        self._stats.add("drain", now - t_d0)

    # ------------------------------------------------------------------
    # settings-driven distributed placement (dist_mode fanout/stage):
    # the reference wires its parallelism entirely through config
    # (container/config/parser_settings.yaml out_addr); here torchrun +
    # one YAML places the same topology across ranks/GPUs with RCCL
    # collectives (gloo on CPU) instead of socket hops.
    # ------------------------------------------------------------------
    def _run_dist_loop(self) -> None:
        import torch
        import torch.distributed as tdist

        from ..parallel import dist as dmx_dist

        ctx = self._dist_ctx
        device = torch.device("cpu")
        if tdist.get_backend() == "nccl":
            device = torch.device("cuda", torch.cuda.current_device())
        mode, rank, world = ctx.mode, ctx.rank, ctx.world
        src = ctx.src if mode == "fanout" else 0
        head = rank == src
        self._log.info(
            "engine DIST loop started: mode=%s rank=%d/%d src=%d head=%s",
            mode, rank, world, src, head)
        if head:
            degraded = self._dist_head_loop(dmx_dist, mode, rank, world,
                                            device)
        else:
            degraded = self._dist_sink_loop(dmx_dist, mode, rank, world,
                                            src, device)
        if degraded and not self._stop_event.is_set():
            # elastic degradation (SURVEY §5.8 hard part): a dead peer
            # broke the collective path — keep serving through the plain
            # socket loop (own engine_addr in, out_addr fan-out, retry-
            # then-drop) instead of going dark. Peers that come back
            # rejoin at the next service restart (communicator reform is
            # parallel/elastic.py's mechanism).
            self._log.warning("dist peer lost: degrading to the socket loop")
            self.metrics.engine_dist_degraded.inc()
            return self._run_socket_loop()
        self._log.info("engine dist loop exited")

    def _dist_process(self, frames: List[bytes]) -> List[bytes]:
        """What the head and the sink do with a non-empty batch: count it
        read, process under the error guard, count it processed (also
        after an error, which yields no outputs). None results drop."""
        n_bytes = sum(len(f) for f in frames)
        self._count_read(n_bytes, len(frames))
        t0 = time.perf_counter()
        try:
            outs = [o for o in self.processor.process_batch(frames)
                    if o is not None]
        except Exception as exc:  # noqa: BLE001
            self.metrics.processing_errors_total.inc(len(frames))
            self._log.error("dist processing error: %s", exc)
            outs = []
        self._count_processed(n_bytes, len(frames), time.perf_counter() - t0)
        return outs

    def _dist_head_loop(self, dmx_dist, mode, rank, world, device) -> bool:
        """Returns True when the collective path failed (degrade)."""
        s = self.settings
        degraded = False
        while not self._stop_event.is_set():
            try:
                frames = self._pair_sock.recv_many(
                    s.engine_batch_size, s.engine_recv_timeout,
                    s.engine_batch_linger_ms)
            except RecvTimeout:
                frames = []
            except SocketClosed:
                break
            frames = [f for f in frames if f]
            outs = self._dist_process(frames) if frames else []
            flag = dmx_dist.FRAME_DATA if outs else dmx_dist.FRAME_HEARTBEAT
            try:
                if mode == "fanout":
                    dmx_dist.broadcast_frames_src(outs, rank, device, flag)
                else:
                    dmx_dist.send_frames(outs, rank + 1, device, flag)
            except RuntimeError as exc:
                self._log.error("dist send failed (peer lost?): %s", exc)
                degraded = True
                break
            for out in outs:
                self._count_written(out, True, 1)
        # wake every peer out of its collective before exiting
        try:
            if mode == "fanout":
                dmx_dist.broadcast_frames_src([], rank, device,
                                              dmx_dist.FRAME_SHUTDOWN)
            else:
                dmx_dist.send_frames([], rank + 1, device,
                                     dmx_dist.FRAME_SHUTDOWN)
        except RuntimeError:
            pass
        return degraded

    def _dist_sink_loop(self, dmx_dist, mode, rank, world, src,
                        device) -> bool:
        """Returns True when the collective path failed (degrade)."""
        last = mode == "fanout" or rank == world - 1
        degraded = False
        while not self._stop_event.is_set():
            try:
                if mode == "fanout":
                    frames, flag = dmx_dist.broadcast_frames_sink(src, device)
                else:
                    frames, flag = dmx_dist.recv_frames(rank - 1, device)
            except RuntimeError as exc:
                self._log.error("dist recv failed (peer lost?): %s", exc)
                degraded = True
                break
            if flag == dmx_dist.FRAME_SHUTDOWN:
                if mode == "stage" and rank + 1 < world:
                    try:
                        dmx_dist.send_frames([], rank + 1, device,
                                             dmx_dist.FRAME_SHUTDOWN)
                    except RuntimeError:
                        pass
                break
            outs = self._dist_process(frames) if frames else []
            if mode == "stage" and not last:
                flag = (dmx_dist.FRAME_DATA if outs
                        else dmx_dist.FRAME_HEARTBEAT)
                try:
                    dmx_dist.send_frames(outs, rank + 1, device, flag)
                except RuntimeError as exc:
                    self._log.error("dist forward failed: %s", exc)
                    degraded = True
                    break
                for out in outs:
                    self._count_written(out, True, 1)
            else:
                for out in outs:
                    self._send_to_outputs(out)
        return degraded

    def _run_source_loop(self) -> None:
        """Source mode: the component generates frames (reader services).

        The input socket stays bound (admin/back-channel parity) but the
        data flows component → outputs."""
        s = self.settings
        gen = self.processor.source_batches(s.engine_batch_size, self._stop_event)
        self._log.info("engine source loop started (outputs=%d)", len(self._out_socks))
        for batch in gen:
            if self._stop_event.is_set():
                break
            t0 = time.perf_counter()
            n_bytes = sum(len(f) for f in batch)
            n_lines = sum(_count_lines(f) for f in batch)
            self._count_read(n_bytes, n_lines, len(batch))
            for out in batch:
                self._send_to_outputs(out)
            # "processing" a generated batch is sending it on
            self._count_processed(n_bytes, n_lines, time.perf_counter() - t0)
        self._log.info("engine source loop exited")

    def _send_to_outputs(self, data: bytes) -> None:
        """Broadcast to all outputs with retry-then-drop per socket
        (reference engine.py:266-302)."""
        for sock in self._out_socks:
            sent = False
            for _attempt in range(self.settings.engine_retry_count):
                try:
                    if sock.send(data, block=False):
                        sent = True
                        break
                except SocketClosed:
                    break
                time.sleep(0.01)
            self._count_written(data, sent)
            if not sent:
                self._log.debug("dropped frame for %s", sock.addr)
