"""The congruences of tests/dlog_decrypt.py against oracle/saver.py: a ciphertext built from known logs for a chosen message decrypts
to it under the oracle's own pairing, and the model's reasons are the oracle's verdicts.  msg_size 1 and ten Miller loops: the model is
what the GPU tests trust in place of the oracle."""
import bls12_381 as o
import saver as sv

import dlog_decrypt as dd
from dlog_election import rng as make_rng


def test_a_known_log_ciphertext_decrypts_to_its_message_under_the_oracle():
    rg = make_rng(31)
    key = dd.DecryptKey(rg, 1)
    us = key.ciphertext([5], rg)
    ct = [o.g1_from_limbs(x) for x in dd.ct_batch(key, [us])[0]]
    vk, gabc = key.oracle_vk(), key.oracle_gamma_abc()
    msgs, nu = sv.decrypt(key.rho, vk, gabc, ct, max_value=8)
    assert msgs == [5] and key.decrypt(us, 8) == ([5], [0]) and key.decrypt(us, 4) == ([dd.NONE], [1])
    assert nu == o.G1.mul(o.G1.gen, key.rho * us[0] % o.R)
    assert key.reason(us, [5], key.rho * us[0]) == (0, 0xFFFFFFFF) and sv.verify_decryption(vk, gabc, ct, [5], nu)
    assert key.reason(us, [6], key.rho * us[0]) == (4, 0) and not sv.verify_decryption(vk, gabc, ct, [6], nu)
    assert key.reason(us, [5], key.rho * us[0] + 1) == (6, 0) and key.reason(us, [o.R], key.rho * us[0]) == (1, 0xFFFFFFFF)
    # an arbitrary member has the logarithm the model states: built for -1, it is r - 1
    assert key.slot_log(key.ciphertext([o.R - 1], rg), 0) == o.R - 1
