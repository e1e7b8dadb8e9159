"""The host's choice of the ingest kernel for one push (fw_host_ig_pack_choice, fw_api.hip), as a table.

k_ingest_pack never folds.  In the default mode (FW_IG_PACK=1) a push of an eligible handle packs
unless something has to be folded or measured: the ingest mirror is invalid or lacks the fold-skip
or the PF_PACK bit; no merge has been launched since the control block was initialised (no flush
epoch can carry PF_PACK fields yet); or a fold measurement is due -- 64 pushes after the last push
on which k_ingest folded, 8 while the packing kernel's sampled estimate (the skew bit) says the
stream folds.  Only that last case tells k_ingest to fold whatever its push count is (FW_IG_FOLD)."""
import pytest

from flink_amd import _native

INGEST, PACK, FOLD = 0, 1, 2                 # FW_IG_INGEST / FW_IG_PACK / FW_IG_FOLD
FOLD_SKIP, PK_OK, SKEW = 1, 2, 4             # mirror bits
X_PLAN, X_KEY_HASH, X_SEGMENTS, X_STRIDE, X_FOLD_ALWAYS = 1, 2, 4, 8, 16
INVALID = (1 << 64) - 1
GOOD = (37 << 8) | FOLD_SKIP | PK_OK         # a mirror word after push 37 of a uniform stream


def choice(mode, mirror, since, merges, inel=0):
    return int(_native.lib().fw_host_ig_pack_choice(mode, mirror, since, merges, inel))


TABLE = [
    # mode, mirror, pushes since the fold, merge launches, ineligible, expected
    (1, GOOD, 1, 1, 0, PACK),
    (1, GOOD, 63, 5, 0, PACK),
    (1, GOOD, 64, 5, 0, FOLD),
    (1, GOOD, 1000, 5, 0, FOLD),
    (1, GOOD | SKEW, 7, 5, 0, PACK),
    (1, GOOD | SKEW, 8, 5, 0, FOLD),
    (1, GOOD | SKEW, 64, 5, 0, FOLD),
    (1, GOOD, 8, 5, 0, PACK),                      # 8 pushes without the skew bit: no measurement due
    (1, INVALID, 1, 5, 0, INGEST),                 # nothing reported yet
    (1, GOOD & ~FOLD_SKIP, 1, 5, 0, INGEST),       # the LDS fold is on: k_ingest folds as it is
    (1, GOOD & ~PK_OK, 1, 5, 0, INGEST),           # no valid PF_PACK fields
    (1, (37 << 8) | SKEW, 100, 5, 0, INGEST),      # neither bit: not a fold request either
    (1, GOOD, 1, 0, 0, INGEST),                    # first flush epoch: nothing can pack yet
    (1, GOOD, 64, 0, 0, INGEST),                   # ... and no forced fold there (k_ingest's own every-8th holds)
    (1, GOOD | SKEW, 8, 0, 0, INGEST),
    (0, GOOD, 1, 5, 0, INGEST),                    # FW_IG_PACK=0: never
    (0, GOOD, 64, 5, 0, INGEST),
    (0, INVALID, 0, 0, 0, INGEST),
    (2, GOOD, 1, 5, 0, PACK),                      # FW_IG_PACK=2: every push of an eligible handle
    (2, INVALID, 0, 0, 0, PACK),
    (2, GOOD & ~FOLD_SKIP, 64, 0, 0, PACK),
    (2, GOOD | SKEW, 8, 5, 0, PACK),
    (2, GOOD, 1, 5, X_FOLD_ALWAYS, PACK),          # FW_FOLD=1 does not stop mode 2
    (1, GOOD, 1, 5, X_FOLD_ALWAYS, INGEST),        # ... but keeps k_ingest in mode 1 (it folds every push as it is)
    (1, GOOD, 64, 5, X_FOLD_ALWAYS, INGEST),
]


@pytest.mark.parametrize("mode,mirror,since,merges,inel,want", TABLE)
def test_choice_table(mode, mirror, since, merges, inel, want):
    assert choice(mode, mirror, since, merges, inel) == want


@pytest.mark.parametrize("flag", [X_PLAN, X_KEY_HASH, X_SEGMENTS, X_STRIDE])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_each_ineligible_flag_keeps_k_ingest(mode, flag):
    """The handle's plan, precomputed key hashes, padded segments and packed rows: never packed, never
    told to fold, in any mode and whatever the mirror says."""
    for mirror in (GOOD, GOOD | SKEW, INVALID):
        for since in (1, 8, 64):
            assert choice(mode, mirror, since, 5, flag) == INGEST
            assert choice(mode, mirror, since, 5, flag | X_FOLD_ALWAYS) == INGEST


def test_thresholds_are_exact():
    """63 against 64 pushes since the fold; 7 against 8 with the skew bit."""
    assert [choice(1, GOOD, s, 1) for s in (62, 63, 64, 65)] == [PACK, PACK, FOLD, FOLD]
    assert [choice(1, GOOD | SKEW, s, 1) for s in (6, 7, 8, 9)] == [PACK, PACK, FOLD, FOLD]


def test_push_count_bits_do_not_matter():
    """The word's push count (bits 8..) is not part of the choice: the every-8th rule is k_ingest's own."""
    for count in (0, 7, 8, 16, 1 << 20):
        assert choice(1, (count << 8) | FOLD_SKIP | PK_OK, 3, 1) == PACK


def test_symbol_is_declared_and_bound():
    assert "fw_host_ig_pack_choice" in _native.EXPORTED
