"""CPU: the host decisions the device-chain drivers share (no kernels) -- pipeline._chain_verdict against the nested `if`s the one-frame
driver carried before the drivers shared it, over every combination of the four flag bits and the guard of each round; which guards it
asks and when it reports a round's estimate; the result it assembles; and pipeline._guard_slot for every driver's ring."""
import itertools

import pytest

from yond_public_amd import _lib as L
from yond_public_amd import engine as E
from yond_public_amd import pipeline as P

FLAGS = range(16)                       # PRM_NO_FLAT_AREA | PRM_LUT_CAPACITY | PRM_ROUND_ABORTED | PRM_BAD_ESTIMATE: every subset
ROUND = list(itertools.product(FLAGS, (False, True)))


def model(rounds):
    """_iter_denoise_chain as it stood with the decision written out: (verdict, the rounds whose estimate it logged, the guards it read)."""
    logged, asked = [], []
    fl1, trip1 = rounds[0]
    two = len(rounds) == 2
    if fl1 & (P.PRM_NO_FLAT_AREA | P.PRM_LUT_CAPACITY | P.PRM_BAD_ESTIMATE):
        return 'host', logged, asked
    asked.append(0)
    if trip1:
        return 'host', logged, asked
    logged.append(0)
    kept = 1
    if two:
        fl2, trip2 = rounds[1]
        if fl2 & (P.PRM_NO_FLAT_AREA | P.PRM_LUT_CAPACITY):
            return 'host', logged, asked
        logged.append(1)
        if not (fl2 & P.PRM_ROUND_ABORTED):
            if fl2 & P.PRM_BAD_ESTIMATE:
                return 'host', logged, asked
            asked.append(1)
            if trip2:
                return 'host', logged, asked
            kept = 2
    return ('both' if kept == len(rounds) else 'round1'), logged, asked


def run(rounds):
    """_chain_verdict with counting callables for the guards: (verdict, rounds reported, guards asked)."""
    logged, asked = [], []

    def guard(r, value):
        def tripped():
            asked.append(r)
            return value
        return tripped
    v = P._chain_verdict([(fl, guard(r, t)) for r, (fl, t) in enumerate(rounds)], logged.append)
    return v, logged, asked


def test_flag_bits_are_the_four_the_cases_enumerate():
    assert sorted((P.PRM_NO_FLAT_AREA, P.PRM_LUT_CAPACITY, P.PRM_ROUND_ABORTED, P.PRM_BAD_ESTIMATE)) == [1, 2, 4, 8]


def test_two_round_verdict_all_1024_cases():
    n = 0
    for r1, r2 in itertools.product(ROUND, ROUND):
        want = model([r1, r2])
        assert run([r1, r2]) == want, (r1, r2)
        assert P._chain_verdict([r1, r2]) == want[0], (r1, r2)                 # plain bools, no hook
        n += 1
    assert n == 1024


def test_one_round_verdict_all_32_cases():
    for r1 in ROUND:
        want = model([r1])
        assert want[0] in ('host', 'both')
        assert run([r1]) == want, r1
        assert P._chain_verdict([r1]) == want[0], r1
    assert len(ROUND) == 32


def test_round2_guard_is_not_read_when_the_answer_does_not_depend_on_it():
    """_Guard.tripped waits for the forward it watched: round 2's is left alone when round 1 already sends the frame to the host, when round 2's
    estimate is unusable, and when round 2 was aborted (its forward computed nothing that is kept); round 1's when its flags decide."""
    for r1, r2 in itertools.product(ROUND, ROUND):
        v, _, asked = run([r1, r2])
        bad1 = bool(r1[0] & (P.PRM_NO_FLAT_AREA | P.PRM_LUT_CAPACITY | P.PRM_BAD_ESTIMATE))
        assert (0 in asked) == (not bad1)
        if bad1 or r1[1] or r2[0] & (P.PRM_NO_FLAT_AREA | P.PRM_LUT_CAPACITY | P.PRM_ROUND_ABORTED | P.PRM_BAD_ESTIMATE):
            assert 1 not in asked, (r1, r2)
        else:
            assert asked == [0, 1] and v == ('host' if r2[1] else 'both')
        assert len(asked) == len(set(asked))                                   # each guard at most once
    assert run([(0, False), (P.PRM_ROUND_ABORTED | P.PRM_BAD_ESTIMATE, True)]) == ('round1', [0, 1], [0])


def test_chain_answer_keeps_the_rounds_the_verdict_names():
    blocks = [(('b1', 'b2'), ('K', 's'), 0, {'th': 1.0}), (('c1', 'c2'), ('K2', 's2'), 0, {'th': 2.0})]
    outs = ['out1', 'out2']
    assert P._chain_answer('host', outs, blocks) is None
    assert P._chain_answer('round1', outs, blocks) == dict(raw_dns=['out1'], regs=[('b1', 'b2')], params=[('K', 's')], nle_info={'th': 1.0})
    assert P._chain_answer('both', outs, blocks) == dict(raw_dns=outs, regs=[('b1', 'b2'), ('c1', 'c2')], params=[('K', 's'), ('K2', 's2')],
                                                         nle_info={'th': 1.0})
    assert P._chain_answer('both', outs[:1], blocks[:1]) == dict(raw_dns=['out1'], regs=[('b1', 'b2')], params=[('K', 's')], nle_info={'th': 1.0})


def rings(lanes):
    """Per driver: (name, ring, words per frame, rounds, the slot as the driver wrote it out before _guard_slot)."""
    once = lambda k, r, ring: 4 + k % ring
    pair = lambda k, r, ring: 4 + 2 * (k % ring) + r
    return [('_denoise_stream_chain', lanes + 2, 1, 1, once), ('denoise_stream_batches', lanes + 2, 1, 1, once),
            ('_denoise_lanes, once', lanes + 2, 2, 1, pair), ('_denoise_lanes, iter', lanes + 2, 2, 2, pair),
            ('_denoise_stream_chain_iter', 4, 2, 2, pair), ('denoise_stream_groups', 4, 2, 2, pair)]


@pytest.mark.parametrize("lanes", [1, 2])
def test_guard_slots_of_every_driver(lanes):
    """64 consecutive frames: the slot is the driver's former literal formula, lies in the ring's part of the status words, and the frames
    that can be live together -- any `ring` consecutive ones: a frame's words rest until it has been yielded -- have distinct slots."""
    assert E.STATUS_WORDS == 12
    for name, ring, per_frame, rounds, formula in rings(lanes):
        slots = [[P._guard_slot(k, ring, r, per_frame) for r in range(rounds)] for k in range(64)]
        for k in range(64):
            for r in range(rounds):
                assert slots[k][r] == formula(k, r, ring), (name, k, r)
                assert 4 <= slots[k][r] < E.STATUS_WORDS, (name, k, r)
        for k in range(64 - ring + 1):
            window = [s for fr in slots[k:k + ring] for s in fr]
            assert len(window) == len(set(window)), (name, k)


def test_a_ring_that_does_not_fit_the_status_words_is_refused():
    """STREAM_LANES 3 with lane pipelines: a ring of 5 frames of 2 words reaches word 13 of 12 at its fifth frame -- refused at the first."""
    for r in range(2):
        for k in range(64):
            with pytest.raises(L.YondHipError):
                P._guard_slot(k, 3 + 2, r, 2)
    assert [P._guard_slot(k, 3 + 2) for k in range(5)] == [4, 5, 6, 7, 8]     # (one word per frame: three lanes fit)
    with pytest.raises(L.YondHipError):
        P._guard_slot(0, 9)
    for slot in (-1, E.STATUS_WORDS, 13):
        with pytest.raises(L.YondHipError):
            P._Guard(None, slot)                                               # (refused before the plan is touched)
