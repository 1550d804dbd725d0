"""The cfx_dist_* exchange primitives of one rank against a model of all its peers, in one process.

A communicator is (world, rank, callback): the callback is handed every segment of an exchange and has to move the
bytes.  `ModelPeers` owns such a callback and plays every peer: it records what the library hands it per segment (the
peer rank and the bytes to send) and fills every receive part with bytes that the test prepared.  So one process drives
rank 1 of a world of 4 (peers 0, 2 and 3) through both callback transports -- host-staged (cfx_dist_comm_create_host: the
segments arrive in pinned host memory) and device (cfx_dist_comm_create_device: they arrive as HBM pointers).

The reference is a numpy model of the contract in include/cutfemx_amd.h (cfx_dist_exchange): what is sent is x[send]
taken BEFORE anything is combined, what arrives is combined in segment order, entries outside every receive part keep
their bits.  An exchange is a copy, one IEEE addition per entry and segment, or a 0/1 OR, so every comparison is
bit-exact (bytes of the float64 / int8 arrays); no tolerance is involved.  Arrays start from random bit patterns
(float64 copies: any pattern, NaNs included; additions: finite values of mixed sign and magnitude where something is
added, any pattern elsewhere)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WORLD, RANK = 4, 1
N = 1500                                   # elements of the exchanged arrays (<= 2000)
COUNTS = [0, 1, 255, 256, 257, 1000]       # around the 256-thread block of the pack / combine kernels, and several blocks
OPS = ["forward", "add", "or", "ind_forward"]
OP_DTYPE = {"forward": np.float64, "add": np.float64, "or": np.int8, "ind_forward": np.int8}
OP_ENTRY = {"forward": "cfx_dist_scatter_forward", "add": "cfx_dist_scatter_reverse_add", "or": "cfx_dist_indicator_or",
            "ind_forward": "cfx_dist_indicator_forward"}


class ModelPeers:
    """All peers of one rank.  `replies` holds, per expected callback call and in order, the bytes that arrive in each
    segment; `calls` records per call [(peer, bytes handed over for sending, size of the receive part), ...]."""

    def __init__(self, transport, world=WORLD, rank=RANK):
        import torch

        from cutfemx_amd import _lib
        self.torch, self._lib, self.l = torch, _lib, _lib.lib()
        self.transport, self.world, self.rank = transport, world, rank
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.calls, self.replies, self.errors, self.fail_next = [], [], [], False
        self._cb = _lib.HOST_EXCHANGE_FN(self._exchange)         # (kept alive with the communicator)
        self.h = C.c_void_p()
        create = self.l.cfx_dist_comm_create_host if transport == "host" else self.l.cfx_dist_comm_create_device
        _lib.check(create(world, rank, self._cb, None, C.byref(self.h)))

    # the two transports differ only in where the segments live: pinned host memory or HBM (read and written the way
    # cutfemx_amd.dist does it: as_torch views, .cpu(), copy_)
    def _read(self, ptr, nbytes):
        if nbytes == 0:
            return b""
        if self.transport == "host":
            return C.string_at(ptr, nbytes)
        from cutfemx_amd.dist import as_torch
        return as_torch(ptr, nbytes, "uint8", self.dev).cpu().numpy().tobytes()

    def _write(self, ptr, data):
        if len(data) == 0:
            return
        if self.transport == "host":
            C.memmove(ptr, data, len(data))
            return
        from cutfemx_amd.dist import as_torch
        as_torch(ptr, len(data), "uint8", self.dev).copy_(self.torch.frombuffer(bytearray(data), dtype=self.torch.uint8))

    def _exchange(self, _user, n, peers, send, send_bytes, recv, recv_bytes):
        try:
            # every send part is read before any receive part is written
            self.calls.append([(int(peers[i]), self._read(send[i], int(send_bytes[i])), int(recv_bytes[i]))
                               for i in range(n)])
            if self.fail_next:
                self.fail_next = False
                return 1
            reply = self.replies.pop(0) if n > 0 else []
            assert len(reply) == n, f"{n} segments, {len(reply)} prepared"
            for i in range(n):
                assert len(reply[i]) == int(recv_bytes[i]), f"segment {i}: {recv_bytes[i]} bytes asked, {len(reply[i])} prepared"
                self._write(recv[i], reply[i])
            if self.transport == "device":
                self.torch.cuda.current_stream().synchronize()
            return 0
        except Exception as e:            # (an exception must not cross the C frame)
            import traceback
            traceback.print_exc()
            self.errors.append(repr(e))
            return 1

    def exchanges(self, segs):
        """[(peer, send part, recv part), ...] -> (cfx_dist_exchange array, objects to keep alive); a part is
        ("range", offset, count) or ("index", int32 numpy list), the list uploaded to HBM"""
        arr = (self._lib.DistExchange * max(len(segs), 1))()
        keep = []
        for i, (peer, snd, rcv) in enumerate(segs):
            arr[i].peer = peer
            for side, part in (("send", snd), ("recv", rcv)):
                if part[0] == "range":
                    setattr(arr[i], side + "_offset", part[1])
                    setattr(arr[i], side + "_count", part[2])
                else:
                    # (an empty list still gets a device address, so that the call takes the index-list form)
                    host = part[1] if part[1].size else np.zeros(1, dtype=np.int32)
                    t = self.torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(self.dev)
                    keep.append(t)
                    setattr(arr[i], side + "_index", t.data_ptr())
                    setattr(arr[i], side + "_count", int(part[1].size))
        return arr, keep

    def upload(self, host):
        t = self.torch.from_numpy(host.copy()).to(self.dev)
        self.torch.cuda.synchronize()
        return t

    def download(self, t):
        self._lib.check(self.l.cfx_synchronize())
        self.torch.cuda.synchronize()
        return t.cpu().numpy()

    def close(self):
        if self.h:
            self._lib.check(self.l.cfx_dist_comm_destroy(self.h))
            self.h = None


@pytest.fixture(params=["host", "device"])
def peers(request):
    mp = ModelPeers(request.param)
    yield mp
    mp.close()
    assert not mp.errors, mp.errors


# ---- the numpy model of the contract ---------------------------------------------------------------------------------
def part_index(part):
    return np.arange(part[1], part[1] + part[2], dtype=np.int64) if part[0] == "range" else part[1].astype(np.int64)


def model(op, x, segs, incoming):
    """(what each segment sends, the array afterwards)"""
    sent = [x[part_index(snd)].copy() for _, snd, _ in segs]           # before anything is combined
    y = x.copy()
    for (_, _, rcv), inc in zip(segs, incoming):                       # in segment order
        r = part_index(rcv)
        if op in ("forward", "ind_forward"):
            y[r] = inc
        elif op == "add":
            y[r] = y[r] + inc
        else:
            y[r] = ((y[r] != 0) | (inc != 0)).astype(np.int8)
    return sent, y


def any_f64(rng, n):
    return rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64)


def finite_f64(rng, n):
    """random sign and mantissa, exponents 2^-30 .. 2^30: sums round, cancel and never leave the finite range"""
    bits = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)) \
        | (rng.integers(1023 - 30, 1023 + 31, n, dtype=np.uint64) << np.uint64(52)) | rng.integers(0, 2 ** 52, n, dtype=np.uint64)
    return bits.view(np.float64)


def any_i8(rng, n):
    return rng.integers(-128, 128, n, dtype=np.int8)


def flags_i8(rng, n):
    """indicator entries as a caller may leave them: mostly 0 / 1, some other non-zero values"""
    return rng.choice(np.array([0, 0, 0, 0, 1, 1, 5, -1, -128, 127], dtype=np.int8), n)


def make_arrays(rng, op, n, segs):
    """(x, [incoming per segment])"""
    touched = np.zeros(n, dtype=bool)
    for _, _, rcv in segs:
        touched[part_index(rcv)] = True
    counts = [part_index(rcv).size for _, _, rcv in segs]
    if op == "forward":
        return any_f64(rng, n), [any_f64(rng, c) for c in counts]
    if op == "add":
        return np.where(touched, finite_f64(rng, n), any_f64(rng, n)), [finite_f64(rng, c) for c in counts]
    if op == "ind_forward":
        return any_i8(rng, n), [any_i8(rng, c) for c in counts]
    return np.where(touched, flags_i8(rng, n), any_i8(rng, n)), [flags_i8(rng, c) for c in counts]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def unsorted_list(rng, pool, count):
    """`count` distinct entries of `pool` in random, not ascending, order"""
    idx = rng.permutation(np.asarray(pool))[:count].astype(np.int32)
    if count >= 2 and np.all(np.diff(idx) > 0):
        idx = idx[::-1].copy()
    return idx


def make_part(rng, kind, count, offset, pool=None):
    if kind == "range":
        return ("range", offset, count)
    return ("index", unsorted_list(rng, np.arange(N) if pool is None else pool, count))


def run_exchange(mp, op, x_host, segs, incoming):
    """One exchange call of rank 1 against the model peers: the bytes handed to the transport (pack) and the array
    afterwards (combine) must equal the numpy model bit for bit.  Returns the array afterwards."""
    assert x_host.dtype == OP_DTYPE[op]
    x = mp.upload(x_host)
    ex, keep = mp.exchanges(segs)
    mp.replies.append([inc.tobytes() for inc in incoming])
    before = len(mp.calls)
    code = getattr(mp.l, OP_ENTRY[op])(mp.h, C.c_void_p(x.data_ptr()), len(segs), ex)
    assert code == 0, (code, mp.l.cfx_last_error())
    got = mp.download(x)
    del keep
    assert not mp.errors, mp.errors
    assert len(mp.calls) == before + 1 and not mp.replies
    sent_want, x_want = model(op, x_host, segs, incoming)
    call = mp.calls[-1]
    assert [c[0] for c in call] == [s[0] for s in segs]
    for i, ((_, sent, recv_bytes), want, inc) in enumerate(zip(call, sent_want, incoming)):
        assert sent == want.tobytes(), f"segment {i}: the bytes handed to the transport are not x[send]"
        assert recv_bytes == inc.nbytes
    bits = np.int64 if got.dtype == np.float64 else np.int8
    assert same_bits(got, x_want), f"{int((got.view(bits) != x_want.view(bits)).sum())} entries differ from the model"
    return got


# ---- one segment: layouts x counts x ops -----------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("recv_kind", ["range", "index"])
@pytest.mark.parametrize("send_kind", ["range", "index"])
@pytest.mark.parametrize("op", OPS)
def test_one_segment(peers, op, send_kind, recv_kind, count):
    """Send and receive side each contiguous (odd offsets) or an unsorted duplicate-free index list, counts on both
    sides of the 256-thread block; float64 copy / add and int8 copy / OR (int8 through index lists included)."""
    rng = np.random.default_rng([COUNTS.index(count), OPS.index(op), int(send_kind == "index"), int(recv_kind == "index")])
    peer = [0, 2, 3][COUNTS.index(count) % 3]
    segs = [(peer, make_part(rng, send_kind, count, 7), make_part(rng, recv_kind, count, 311))]
    x, incoming = make_arrays(rng, op, N, segs)
    got = run_exchange(peers, op, x, segs, incoming)
    if op == "or":
        assert set(np.unique(got[part_index(segs[0][2])])) <= {0, 1}


@pytest.mark.parametrize("recv_kind", ["range", "index"])
@pytest.mark.parametrize("send_kind", ["range", "index"])
@pytest.mark.parametrize("op", ["forward", "add"])
@pytest.mark.parametrize("send_count,recv_count", [(257, 100), (3, 300), (0, 257), (300, 0)])
def test_send_count_differs_from_receive_count(peers, op, send_kind, recv_kind, send_count, recv_count):
    rng = np.random.default_rng([send_count, recv_count, int(op == "add"), int(send_kind == "index"), int(recv_kind == "index")])
    segs = [(3, make_part(rng, send_kind, send_count, 5), make_part(rng, recv_kind, recv_count, 401))]
    x, incoming = make_arrays(rng, op, N, segs)
    run_exchange(peers, op, x, segs, incoming)


def three_segments(rng):
    """Two segments to peer 2 and one to peer 3 with pairwise disjoint receive parts; send parts overlap receive parts
    (segment 1 sends entries that segment 0 overwrites: what is sent is the value from before).  Segment 0 is the
    largest on both sides."""
    pool = rng.permutation(np.arange(400, N))
    return [(2, ("index", unsorted_list(rng, np.arange(N), 300)), ("range", 91, 280)),
            (2, ("range", 101, 13), ("index", pool[:257].astype(np.int32))),
            (3, ("index", unsorted_list(rng, np.arange(80, 400), 40)), ("index", pool[257:258].astype(np.int32)))]


@pytest.mark.parametrize("op", OPS)
def test_two_segments_to_one_peer_and_one_to_another(peers, op):
    rng = np.random.default_rng([3, OPS.index(op)])
    segs = three_segments(rng)
    x, incoming = make_arrays(rng, op, N, segs)
    run_exchange(peers, op, x, segs, incoming)


@pytest.mark.parametrize("second", ["index", "range"])
def test_reverse_add_receive_parts_share_entries(peers, second):
    """Two segments from different peers add into the same entries: the additions happen in segment order
    ((x + a) + b, rounded twice), bit for bit."""
    rng = np.random.default_rng([4, int(second == "index")])
    first = unsorted_list(rng, np.arange(N), 300)
    if second == "index":
        part2 = ("index", rng.permutation(np.concatenate([first[:150], unsorted_list(rng, np.setdiff1d(np.arange(N), first), 107)]))
                 .astype(np.int32))
    else:
        part2 = ("range", 333, 257)
    segs = [(0, ("range", 11, 300), ("index", first)), (3, ("index", unsorted_list(rng, np.arange(N), 257)), part2)]
    shared = np.intersect1d(part_index(segs[0][2]), part_index(segs[1][2]))
    assert shared.size > 20
    x, incoming = make_arrays(rng, "add", N, segs)
    got = run_exchange(peers, "add", x, segs, incoming)
    # (the shared entries really saw two roundings somewhere: one fused or reordered sum would differ)
    pos0 = {int(v): k for k, v in enumerate(part_index(segs[0][2]))}
    pos1 = {int(v): k for k, v in enumerate(part_index(segs[1][2]))}
    other = np.array([x[s] + (incoming[0][pos0[int(s)]] + incoming[1][pos1[int(s)]]) for s in shared])
    assert not same_bits(other, got[shared])


# ---- int8 indicators ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,count", [(3, 13), (257, 511)])
@pytest.mark.parametrize("op", ["or", "ind_forward"])
def test_indicator_ranges_at_odd_offsets(peers, op, offset, count):
    """int8 ranges that start and end off every alignment; resident and incoming values other than 0 / 1 (5, -1, -128):
    the OR stores exactly 0 or 1, the copy keeps every byte, the neighbours of the range keep theirs."""
    rng = np.random.default_rng([5, offset, int(op == "or")])
    segs = [(0, ("range", offset + 2, count), ("range", offset, count))]
    x, incoming = make_arrays(rng, op, N, segs)
    if op == "or":      # every combination of (resident, incoming) in {0, 1, 5, -1} occurs
        combos = np.array([(a, b) for a in (0, 1, 5, -1) for b in (0, 1, 5, -1)], dtype=np.int8)[:count]
        x[offset:offset + combos.shape[0]] = combos[:, 0]
        incoming[0][:combos.shape[0]] = combos[:, 1]
    got = run_exchange(peers, op, x, segs, incoming)
    if op == "or":
        assert set(np.unique(got[offset:offset + count])) == {0, 1}
    assert same_bits(got[:offset], x[:offset]) and same_bits(got[offset + count:], x[offset + count:])


# ---- cfx_dist_scatter_reverse_matrix ---------------------------------------------------------------------------------
_MASS = {}


def mass_matrix():
    """The 2D n = 4 P1 mass matrix (25 rows): its pattern handle and host copies of indptr / indices / values."""
    if not _MASS:
        import cutfemx_amd as cfx
        from cutfemx_amd import fem
        mesh = cfx.Mesh.create_box(2, 4)
        V = cfx.FunctionSpace(mesh, 1)
        cells = np.arange(mesh.num_cells, dtype=np.int32)
        A = fem.assemble_matrix(fem.form([fem.Integral(fem.MASS, cells=cells, qdegree=2)], V))
        _MASS.update(A=A, V=V, mesh=mesh, indptr=A.indptr.copy(), indices=A.indices.copy(), values=A.data.copy())
        assert A.nrows == 25
    return _MASS


# (peer, send rows, recv rows): an empty range on either side, a range that ends at the last row on either side; the
# first exchange is the largest
ROW_CASES = {"empty_recv_send_to_last_row": [(0, (0, 8), (8, 16)), (2, (20, 25), (3, 3))],
             "empty_send_recv_to_last_row": [(3, (0, 8), (7, 15)), (0, (4, 4), (20, 25))]}


def row_exchange_array(rows):
    from cutfemx_amd import _lib
    arr = (_lib.DistRowExchange * max(len(rows), 1))()
    for i, (peer, (s0, s1), (r0, r1)) in enumerate(rows):
        arr[i].peer, arr[i].send_row_lo, arr[i].send_row_hi, arr[i].recv_row_lo, arr[i].recv_row_hi = peer, s0, s1, r0, r1
    return arr


def value_segments(indptr, rows):
    return [(peer, ("range", int(indptr[s0]), int(indptr[s1] - indptr[s0])), ("range", int(indptr[r0]), int(indptr[r1] - indptr[r0])))
            for peer, (s0, s1), (r0, r1) in rows]


def handshake(segs, recv_delta=0, send_delta=0, which=None):
    """(what the library sends per segment, what a library on the other side answers): two float64 per segment and
    direction -- (my send count, my receive count) out, the peer's pair in; the peer's send count is my receive count."""
    out = [np.array([s[1][2], s[2][2]], dtype=np.float64).tobytes() for s in segs]
    back = [np.array([s[2][2] + (recv_delta if i == which else 0), s[1][2] + (send_delta if i == which else 0)],
                     dtype=np.float64).tobytes() for i, s in enumerate(segs)]
    return out, back


@pytest.mark.parametrize("case", sorted(ROW_CASES))
def test_matrix_rows_match_model(peers, case):
    """Two row exchanges with different peers on the pattern and values of an assembled matrix.  The model peer answers
    the count handshake as the library on the other side would: per segment the library sends two float64 values, its
    send count and its receive count, and expects the peer's pair (cfx_dist.hip, the block before the value exchange).
    This test pins that wire format: a library that changes it no longer talks to an older one.  Then the value
    slices travel; `values` equals the numpy model bit for bit and the pattern is unchanged."""
    M = mass_matrix()
    rows = ROW_CASES[case]
    rng = np.random.default_rng([6, sorted(ROW_CASES).index(case)])
    segs = value_segments(M["indptr"], rows)
    assert any(s[1][2] == 0 or s[2][2] == 0 for s in segs) and any(r[1][1] == 25 or r[2][1] == 25 for r in rows)
    hs_out, hs_back = handshake(segs)
    incoming = [finite_f64(rng, s[2][2]) for s in segs]
    peers.replies += [hs_back, [inc.tobytes() for inc in incoming]]
    v = peers.upload(M["values"])
    code = peers.l.cfx_dist_scatter_reverse_matrix(peers.h, M["A"]._p, C.c_void_p(v.data_ptr()), len(rows), row_exchange_array(rows))
    assert code == 0, (code, peers.l.cfx_last_error())
    got = peers.download(v)
    assert not peers.errors and len(peers.calls) == 2
    assert [(p, b, r) for p, b, r in peers.calls[0]] == [(s[0], o, 16) for s, o in zip(segs, hs_out)]
    sent_want, want = model("add", M["values"], segs, incoming)
    assert [(p, b, r) for p, b, r in peers.calls[1]] == [(s[0], w.tobytes(), inc.nbytes) for s, w, inc in zip(segs, sent_want, incoming)]
    assert same_bits(got, want)
    assert np.array_equal(M["A"].indptr, M["indptr"]) and np.array_equal(M["A"].indices, M["indices"])
    assert same_bits(M["A"].data, M["values"])          # (the matrix's own values were not the array of this call)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("direction", ["peer_sends_more", "peer_sends_fewer", "peer_expects_more", "peer_expects_fewer"])
def test_matrix_count_mismatch_raises_before_values_travel(peers, direction, which):
    """A peer whose rows hold a different number of entries, in either direction alone: CFX_ERR_RUNTIME after the
    handshake (the peer sees the same pair and raises too), no value exchange follows, `values` keeps its bits."""
    from cutfemx_amd import _lib
    M = mass_matrix()
    rows = [(0, (0, 8), (8, 16)), (2, (20, 25), (16, 20))]
    segs = value_segments(M["indptr"], rows)
    delta = 1 if direction.endswith("more") else -1
    _, hs_back = handshake(segs, recv_delta=delta if "sends" in direction else 0, send_delta=delta if "expects" in direction else 0,
                           which=which)
    peers.replies.append(hs_back)
    v = peers.upload(M["values"])
    code = peers.l.cfx_dist_scatter_reverse_matrix(peers.h, M["A"]._p, C.c_void_p(v.data_ptr()), len(rows), row_exchange_array(rows))
    assert code == _lib.ERR_RUNTIME, (code, peers.l.cfx_last_error())
    assert b"different number of entries" in peers.l.cfx_last_error()
    assert len(peers.calls) == 1 and not peers.errors
    assert same_bits(peers.download(v), M["values"])


@pytest.mark.parametrize("rows", [[(0, (0, 8), (8, 16)), (2, (20, 26), (16, 20))], [(0, (0, 8), (8, 16)), (2, (20, 25), (25, 26))],
                                  [(0, (-1, 8), (8, 16))], [(0, (9, 8), (8, 16))], [(0, (0, 8), (17, 16))]])
def test_matrix_row_range_outside_the_matrix(peers, rows):
    """CFX_ERR_OUT_OF_RANGE before any callback runs (the row pointers of such a range are never read)."""
    from cutfemx_amd import _lib
    M = mass_matrix()
    v = peers.upload(M["values"])
    code = peers.l.cfx_dist_scatter_reverse_matrix(peers.h, M["A"]._p, C.c_void_p(v.data_ptr()), len(rows), row_exchange_array(rows))
    assert code == _lib.ERR_OUT_OF_RANGE, (code, peers.l.cfx_last_error())
    assert not peers.calls
    assert same_bits(peers.download(v), M["values"])


# ---- staging buffers and communicator state --------------------------------------------------------------------------
def test_staging_reused_across_sizes_and_segment_counts(peers):
    """One communicator: small -> 1000 -> small (the pinned staging buffer of a segment slot grows once and is reused),
    then calls with more segments than any call before (new slots appear beside the grown one).  Every call is right."""
    rng = np.random.default_rng(7)
    for k, (op, count) in enumerate([("add", 3), ("forward", 1000), ("add", 5), ("or", 1000), ("ind_forward", 2)]):
        segs = [([0, 2, 3][k % 3], make_part(rng, "index", count, 0), make_part(rng, "range", count, 9 + k))]
        x, incoming = make_arrays(rng, op, N, segs)
        run_exchange(peers, op, x, segs, incoming)
    for op in ("add", "forward"):
        segs = three_segments(rng)
        x, incoming = make_arrays(rng, op, N, segs)
        run_exchange(peers, op, x, segs, incoming)
    pool = rng.permutation(N)
    segs = [(0, ("range", 0, 400), ("index", pool[:400].astype(np.int32))), (2, ("range", 1, 1), ("index", pool[400:401].astype(np.int32))),
            (3, ("index", unsorted_list(rng, np.arange(N), 257)), ("index", pool[401:700].astype(np.int32))),
            (2, ("range", 1100, 399), ("range", 0, 0)), (0, ("range", 0, 0), ("index", pool[700:1099].astype(np.int32)))]
    x, incoming = make_arrays(rng, "add", N, segs)
    run_exchange(peers, "add", x, segs, incoming)


def test_failing_callback_raises_and_the_communicator_goes_on(peers):
    from cutfemx_amd import _lib
    rng = np.random.default_rng(8)
    segs = [(2, make_part(rng, "index", 257, 0), make_part(rng, "index", 300, 0))]
    x_host, incoming = make_arrays(rng, "add", N, segs)
    x = peers.upload(x_host)
    ex, keep = peers.exchanges(segs)
    peers.fail_next = True
    with pytest.raises(RuntimeError, match="callback failed"):
        _lib.check(peers.l.cfx_dist_scatter_reverse_add(peers.h, C.c_void_p(x.data_ptr()), 1, ex))
    assert len(peers.calls) == 1 and not peers.errors
    assert same_bits(peers.download(x), x_host)          # nothing arrived, nothing was combined
    run_exchange(peers, "add", x_host, segs, incoming)
    segs = three_segments(rng)
    x_host, incoming = make_arrays(rng, "forward", N, segs)
    run_exchange(peers, "forward", x_host, segs, incoming)


@pytest.mark.parametrize("op", OPS)
def test_no_segments_and_null_exchange_list(peers, op):
    rng = np.random.default_rng(9)
    x_host = make_arrays(rng, op, 64, [])[0]
    x = peers.upload(x_host)
    assert getattr(peers.l, OP_ENTRY[op])(peers.h, C.c_void_p(x.data_ptr()), 0, None) == 0
    assert same_bits(peers.download(x), x_host)
    assert all(call == [] for call in peers.calls)


# ---- refusals ----------------------------------------------------------------------------------------------------------
REFUSALS = ["peer_negative", "peer_is_world", "peer_is_rank", "send_count_negative", "recv_count_negative", "host_array",
            "host_send_index", "host_recv_index", "bad_peer_in_second_segment"]


@pytest.mark.parametrize("op", ["forward", "or"])
@pytest.mark.parametrize("what", REFUSALS)
def test_refused_with_invalid_argument(peers, what, op):
    """CFX_ERR_INVALID_ARGUMENT; the callback was not called and the array is untouched."""
    from cutfemx_amd import _lib
    rng = np.random.default_rng(10)
    x_host = make_arrays(rng, op, 300, [])[0]
    x = peers.upload(x_host)
    good = (2, ("index", unsorted_list(rng, np.arange(300), 20)), ("index", unsorted_list(rng, np.arange(300), 20)))
    segs = [good, good] if what == "bad_peer_in_second_segment" else [(0, ("range", 3, 10), ("range", 100, 10))]
    ex, keep = peers.exchanges(segs)
    host_index = np.arange(10, dtype=np.int32)
    data = C.c_void_p(x.data_ptr())
    if what.startswith("peer"):
        ex[0].peer = {"peer_negative": -1, "peer_is_world": WORLD, "peer_is_rank": RANK}[what]
    elif what == "send_count_negative":
        ex[0].send_count = -1
    elif what == "recv_count_negative":
        ex[0].recv_count = -1
    elif what == "host_array":
        x_on_host = x_host.copy()
        data = x_on_host.ctypes.data_as(C.c_void_p)
    elif what == "host_send_index":
        ex[0].send_index = host_index.ctypes.data
    elif what == "host_recv_index":
        ex[0].recv_index = host_index.ctypes.data
    else:
        ex[1].peer = RANK
    code = getattr(peers.l, OP_ENTRY[op])(peers.h, data, len(segs), ex)
    assert code == _lib.ERR_INVALID_ARGUMENT, (code, peers.l.cfx_last_error())
    assert not peers.calls
    assert same_bits(peers.download(x), x_host)
    if what == "host_array":
        assert same_bits(x_on_host, x_host)
    del keep
