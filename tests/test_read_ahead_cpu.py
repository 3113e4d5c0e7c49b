"""CPU tests of kitti_data.ReadAhead, the one read-ahead frame feeder: a `prepare` that touches no pinned memory and a stand-in
for the event class, so no device is needed."""
import threading

import pytest

from heterofusionrcnn_amd import kitti_data as KD


class FakeEvent:
    """record() / synchronize() of torch.cuda.Event, counted"""
    recorded, waited = 0, 0

    def record(self):
        FakeEvent.recorded += 1

    def synchronize(self):
        FakeEvent.waited += 1


def _alive(prefix):
    return [t.name for t in threading.enumerate() if t.name.startswith(prefix)]


def _drive(feed, chunks):
    """the consumer's loop: take, "upload", resubmit -> the results in the order they came back"""
    out = []
    feed.submit(chunks[0])
    for i in range(len(chunks)):
        out.append(feed.take())
        feed.uploaded()
        feed.submit(chunks[i + 1] if i + 1 < len(chunks) else None)
    return out


def test_results_in_submit_order_on_two_alternating_stagings():
    FakeEvent.recorded = FakeEvent.waited = 0
    seen, threads = [], set()

    def prepare(picks, staging, pool):
        seen.append(staging)
        threads.add(threading.current_thread().name)
        return list(pool.map(lambda v: 10 * v, picks))

    chunks = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(6)] + [[18]]          # seven chunks, the last one short
    with KD.ReadAhead(prepare, 2, event=FakeEvent) as feed:
        assert _drive(feed, chunks) == [[10 * v for v in c] for c in chunks]
        with pytest.raises(StopIteration):
            feed.take()
    assert all(isinstance(s, KD._Staging) for s in seen) and len({id(s) for s in seen}) == 2
    assert all(seen[i] is seen[i % 2] for i in range(len(seen))) and seen[0] is not seen[1]
    assert len(threads) == 1 and next(iter(threads)).startswith("hf-read")         # the one ahead thread
    # an event per upload; every reuse of a staging (chunks 2..6) waited for the event recorded two uploads earlier
    assert FakeEvent.recorded == len(chunks) and FakeEvent.waited == len(chunks) - 2
    assert _alive("hf-read") == []


def test_take_with_nothing_pending_raises_stop_iteration():
    feed = KD.ReadAhead(lambda picks, staging, pool: picks, 1, event=FakeEvent)
    try:
        with pytest.raises(StopIteration):
            feed.take()
        feed.submit(None)
        with pytest.raises(StopIteration):
            feed.take()
    finally:
        feed.close()


def test_an_exception_in_prepare_is_raised_by_take_and_close_still_returns():
    def prepare(picks, staging, pool):
        return list(pool.map(lambda v: open("/nonexistent-dir/%s.bin" % v, "rb"), picks))

    feed = KD.ReadAhead(prepare, 2, event=FakeEvent)
    feed.submit(["000007"])
    with pytest.raises(FileNotFoundError, match="000007"):
        feed.take()
    feed.close()
    feed.close()                                                                   # twice is fine
    assert _alive("hf-read") == []


def test_close_twice_and_no_reader_thread_survives():
    feed = KD.ReadAhead(lambda picks, staging, pool: list(pool.map(str, picks)), 3, event=FakeEvent)
    assert _drive(feed, [[1, 2, 3], [4, 5, 6]]) == [["1", "2", "3"], ["4", "5", "6"]]
    assert _alive("hf-read")                                                       # pool and ahead threads, named as promised
    feed.close()
    feed.close()
    assert _alive("hf-read") == []
