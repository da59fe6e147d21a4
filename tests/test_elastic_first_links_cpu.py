"""Liveness links of a new generation are up before its first collective.

The links used to be opened by the first heartbeat tick after a generation formed, so a member
killed inside the generation's very first collectives had closed no link yet: the survivors paid a
whole lease, and a fast replacement of the victim was admitted in the same regroup
(tests/test_elastic_midcollective_cpu.py then saw one regroup where it expects two). The guard now
opens them right after the communicator is built, with a bounded wait."""
import time

from tests import _mp


def test_watch_waits_for_reachable_links_and_not_for_refused_ones():
    from distributedvolunteercomputing_amd.parallel.elastic import _P, _Liveness

    port = _mp.free_port()
    store = _mp.make_store(0, 1, port)
    eofs = []
    live = _Liveness(store, 0, "127.0.0.1", lambda m, a: eofs.append(m))
    other = _Liveness(store, 1, "127.0.0.1", lambda m, a: None)
    try:
        live.watch([0, 1], wait_s=5.0)
        assert 1 in live._conn  # established when the call returns: no polling needed
        # a refused connect is not waited for (it proves nothing and is left to the retry)
        store.set(f"{_P}live/2", f"127.0.0.1:{_mp.free_port()}")
        t0 = time.time()
        live.watch([0, 1, 2], wait_s=5.0)
        assert time.time() - t0 < 2.0
        assert 2 not in live._conn and live.connect_failures >= 1
        # a member that has published no address yet is waited for, up to wait_s only
        t0 = time.time()
        live.watch([0, 1, 3], wait_s=0.2)
        assert 0.2 <= time.time() - t0 < 2.0
        # ... and an abort (the guard passes its abort flag) ends that wait at once
        t0 = time.time()
        live.watch([0, 1, 3], wait_s=5.0, give_up=lambda: True)
        assert time.time() - t0 < 1.0
        other.close()
        deadline = time.time() + 5
        while not eofs and time.time() < deadline:
            time.sleep(0.01)
        assert eofs == [1]
    finally:
        live.close()
        other.close()


def _peer(rank, world, port):
    import torch

    from distributedvolunteercomputing_amd.parallel.elastic import ElasticMembership

    store = _mp.make_store(rank, world, port)
    mem = ElasticMembership(store, rank, backend="gloo", lease_s=30.0, heartbeat_s=5.0)
    mem.bootstrap(list(range(world)))
    mem.sync_round()
    with mem.guard():
        # heartbeat_s = 5: no heartbeat tick has run yet, the guard itself opened the links
        linked = sorted(mem._live._conn)
        mem.group.allreduce_(torch.ones(4))
    links_ms = next(e for e in mem.events if e["event"] == "connect")["links_ms"]
    assert links_ms < 500.0, links_ms  # far below link_wait_s: nothing was waited out
    mem.leave()
    store.add("done", 1)
    while rank == 0 and int(store.add("done", 0)) < world:  # the store lives in rank 0
        time.sleep(0.01)
    return linked


def test_first_guard_of_a_generation_opens_the_links():
    out = _mp.run(_peer, 3)
    assert out == {0: [1, 2], 1: [0, 2], 2: [0, 1]}, out
