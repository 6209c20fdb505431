"""st_amd/stepdriver.py on the host: what TrainStep, JointTrainStep and EvalStep share, with stub callables and CPU tensors.

bucket_step is the one place that sets ``functional.TailBuffers.active``; the stubs below record what it holds at every call."""
import contextlib

import pytest
import torch

from st_amd import stepdriver as sd
from st_amd.functional import TailBuffers


# ---- bucket_step ---------------------------------------------------------------------------------------------------------
class _Layout:
    def __init__(self):
        self.valid_rows = torch.zeros(1, dtype=torch.int32)


class _Driver:
    """Recording stand-ins for a driver's eager / capture / replay; the eager call requests one tail buffer, as
    functional.rows_buffer does for a packed layout."""

    def __init__(self, fail=None):
        self.calls, self.active, self.fail, self.layout = [], [], fail, _Layout()

    def _note(self, what):
        self.calls.append(what)
        self.active.append(TailBuffers.active)
        if self.fail == what:
            raise ZeroDivisionError(what)

    def eager(self):
        self._note("eager")
        if TailBuffers.active is not None:
            TailBuffers.active.request(8, 16, self.layout, "cpu")
        return "eager result"

    def capture(self):
        self._note("capture")
        return "cap"

    def replay(self, cap):
        assert cap == "cap"
        self._note("replay")
        return "replay result"


def _bucket():
    st = sd._Bucket()
    st.x = torch.zeros(2, 4, 3)
    return st


def _run(st, drv, packed, w, serve_tails=True):
    out = sd.bucket_step(st, packed, w, drv.eager, drv.capture, drv.replay, serve_tails)
    assert TailBuffers.active is None
    return out


@pytest.mark.parametrize("serve_tails", [True, False])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("w", [0, 1, 2])
def test_bucket_step_sequence_and_tail_buffers(w, packed, serve_tails):
    st, drv = _bucket(), _Driver()
    outs = [_run(st, drv, packed, w, serve_tails) for _ in range(w + 3)]
    assert drv.calls == ["eager"] * w + ["capture", "replay"] + ["replay"] * 2
    assert outs == ["eager result"] * w + ["replay result"] * 3
    assert st.cap == "cap" and st.seen == w + 1
    for i, (what, tb) in enumerate(zip(drv.calls, drv.active)):
        if what == "eager" and i == w - 1 and packed:
            assert tb is st.tails and isinstance(tb, TailBuffers)           # the recording object: the w-th eager call only
        elif what == "capture" and packed and serve_tails and w >= 1:
            assert tb is st.tails and tb.mode == "serve"                     # the materialised object: the capture only
        else:
            assert tb is None, (i, what)
    if packed and w >= 1:
        assert st.tails.specs == [(8, 16, drv.layout)]
        if serve_tails:
            assert [tuple(b.shape) for b in st.tails.bufs] == [(8, 16)] and st.tails.table.shape == (4 * TailBuffers.N_MAX,)
        else:
            assert st.tails.mode == "record" and st.tails.bufs == []
    else:
        assert st.tails is None


def test_bucket_step_resets_active_when_eager_raises():
    st, drv = _bucket(), _Driver(fail="eager")
    with pytest.raises(ZeroDivisionError):
        sd.bucket_step(st, True, 1, drv.eager, drv.capture, drv.replay, True)
    assert isinstance(drv.active[0], TailBuffers) and TailBuffers.active is None and st.cap is None


def test_bucket_step_resets_active_when_capture_raises():
    st, drv = _bucket(), _Driver()
    _run(st, drv, True, 1)
    drv.fail = "capture"
    with pytest.raises(ZeroDivisionError):
        sd.bucket_step(st, True, 1, drv.eager, drv.capture, drv.replay, True)
    assert drv.calls == ["eager", "capture"] and drv.active[1] is st.tails and drv.active[1].mode == "serve"
    assert TailBuffers.active is None and st.cap is None


# ---- LossDenom -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def fills(monkeypatch):
    n = []
    real = torch.Tensor.fill_

    def counted(self, value):
        n.append(float(value))
        return real(self, value)
    monkeypatch.setattr(torch.Tensor, "fill_", counted)
    return n


def test_loss_denom(fills):
    dev = torch.device("cpu")
    d = sd.LossDenom()
    d.stage("tokens", 4, 12, dev)
    d.stage(None, 4, 12, dev)
    assert d.tensor is None and d.host is None and fills == []
    d.stage("rows", 4, 12, dev)
    assert d.tensor.dtype == torch.float32 and d.tensor.tolist() == [48.0]
    ptr = d.tensor.data_ptr()
    del fills[:]                                   # (how torch.full fills is its own affair)
    d.stage("rows", 4, 12, dev)
    d.stage("rows", 6, 8, dev)                     # another batch, the same value
    assert fills == [] and d.tensor.data_ptr() == ptr
    d.stage("rows", 4, 11, dev)
    assert fills == [44.0] and d.tensor.tolist() == [44.0] and d.tensor.data_ptr() == ptr and d.host == 44.0
    s = sd.LossDenom()
    s.stage("sum", 4, 12, dev)
    del fills[:]
    s.stage("sum", 3, 7, dev)
    assert s.tensor.tolist() == [1.0] and fills == []


# ---- batch_signature, trim_batch -----------------------------------------------------------------------------------------
def _raw():
    return (torch.zeros(3, 10, 5), torch.tensor([10, 7, 4]), torch.zeros(3, 6, dtype=torch.long), torch.tensor([6, 2, 3]),
            torch.zeros(3, 6, dtype=torch.long))


def test_batch_signature():
    x, il, tok, tl, gt = raw = _raw()
    sig = sd.batch_signature(*raw)
    assert sig == sd.batch_signature(x, il.clone(), tok, tl.clone(), gt) and hash(sig) == hash(sd.batch_signature(*raw))
    assert sig != sd.batch_signature(x, torch.tensor([10, 7, 5]), tok, tl, gt)            # one length
    assert sig != sd.batch_signature(x, il, tok, torch.tensor([6, 2, 4]), gt)
    assert sig != sd.batch_signature(x[:, :9], il, tok, tl, gt)                            # one shape (the same address)
    assert sig != sd.batch_signature(x, il, tok[:, :5], tl, gt)
    for i in (0, 2, 4):                                                                    # one buffer
        other = list(raw)
        other[i] = raw[i].clone()
        assert sig != sd.batch_signature(*other), i


def test_trim_batch():
    x, il, tok, tl, gt = _raw()
    il, tl = torch.tensor([8, 7, 4]), torch.tensor([4, 2, 3])
    bx, bil, btok, btl, bgt = sd.trim_batch(x, il, tok, tl, gt)
    assert bx.shape == (3, 8, 5) and btok.shape == (3, 4) and bgt.shape == (3, 4) and bil is il and btl is tl
    assert bx.data_ptr() == x.data_ptr() and btok.data_ptr() == tok.data_ptr() and bgt.data_ptr() == gt.data_ptr()


# ---- parse_buckets -------------------------------------------------------------------------------------------------------
def test_parse_buckets():
    assert sd.parse_buckets("TrainStep", None, None) == (None, None)
    assert sd.parse_buckets("TrainStep", [96.0, 12], None) == ((96, 12), None)
    one = sd.parse_buckets("TrainStep", (96, 12), (340, 44))
    assert one == ((96, 12), [(340, 44)]) and one == sd.parse_buckets("TrainStep", (96, 12), [(340, 44)])
    assert one == sd.parse_buckets("TrainStep", (96, 12), [[340.0, 44]])
    assert sd.parse_buckets("EvalStep", (96, 12), [(250, 44), (340, 44)])[1] == [(250, 44), (340, 44)]
    for who in ("TrainStep", "EvalStep"):
        with pytest.raises(ValueError, match=r"^%s: bucket_rows needs bucket=\(T_cap, L_cap\)$" % who):
            sd.parse_buckets(who, None, (340, 44))


def test_drivers_parse_buckets_under_their_own_name():
    from st_amd.evaluate import EvalStep
    from st_amd.trainer import TrainStep

    class Packed(torch.nn.Module):
        def forward_packed(self, *a, **k):
            raise AssertionError("not called")
    with pytest.raises(ValueError, match="^TrainStep: bucket_rows needs"):
        TrainStep(Packed(), None, 30, 5.0, bucket_rows=(340, 44))
    with pytest.raises(ValueError, match="^EvalStep: bucket_rows needs"):
        EvalStep(Packed(), 30, use_graph=False, bucket_rows=(340, 44))


# ---- optimizer_options ---------------------------------------------------------------------------------------------------
class _Optim:
    """The part of ScheduledOptim the drivers read: options_token() and the flag averaged() holds."""

    def __init__(self):
        self._in_averaged, self.guard = False, False

    def options_token(self):
        return (self.guard, None, 0)

    @contextlib.contextmanager
    def averaged(self):
        self._in_averaged = True
        try:
            yield self
        finally:
            self._in_averaged = False


def test_optimizer_options():
    assert sd.optimizer_options(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1), "TrainStep") is None
    opt = _Optim()
    assert sd.optimizer_options(opt, "TrainStep") == (False, None, 0)
    opt.guard = True
    assert sd.optimizer_options(opt, "TrainStep") == (True, None, 0)
    for who in ("TrainStep", "JointTrainStep"):
        with opt.averaged():
            with pytest.raises(RuntimeError, match=r"^%s: called inside optimizer\.averaged\(\)" % who):
                sd.optimizer_options(opt, who)
        assert sd.optimizer_options(opt, who) == (True, None, 0)


def test_trainer_reexports():
    """What tests and tools import from st_amd.trainer is what stepdriver defines."""
    from st_amd import trainer
    for name in ("no_gc_inside_capture", "stage_bucket", "_Bucket"):
        assert getattr(trainer, name) is getattr(sd, name)
    assert "options" in trainer._Captured.__slots__ and callable(trainer.drain_collective_watchdog)
