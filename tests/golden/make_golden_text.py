"""Generate tests/golden/text_ref.npz by calling the REFERENCE's own `random_word`, `random_point_cloud` and
`merge_tokens` (data/data_utils.py:76-104, :107-121, :50-60), imported unmodified from /root/reference (only runnable
in the build container).  A stub tokenizer stands in for BertTokenizer: ids 101 / 102 / 103, vocabulary {str(i): i} for
30 522 ids, and `[CLS] tokens[:max_length - 2] [SEP]` + padding for an already tokenised text (what the real one does to
a string with truncation and padding='max_length').  `random.random` / `random.choice` are wrapped while the reference
runs, so that every draw is recorded at the position where it happened.  Inputs (tests/text_cases.py), draws and the
reference's outputs are stored; no program text.

    python tests/golden/make_golden_text.py
"""
import builtins
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(HERE, "ref_stubs"))
builtins.__POINTNET2_SETUP__ = True

import text_cases as C  # noqa: E402


class StubTokenizer:
    cls_token_id, sep_token_id, mask_token_id, pad_token_id = C.SPECIAL
    vocab = {str(i): i for i in range(C.VOCAB)}

    def __call__(self, tokens, max_length):
        """An already tokenised text -> (input_ids, attention_mask) lists of length max_length."""
        body = [int(t) for t in tokens][:max_length - 2]
        ids = [self.cls_token_id] + body + [self.sep_token_id]
        masks = [1] * len(ids) + [0] * (max_length - len(ids))
        return ids + [self.pad_token_id] * (max_length - len(ids)), masks


class Recorder:
    """Stands in for random.random / random.choice while one reference call runs.  The reference draws once per
    position whose mask is 1, in order, and picks a replacement right after that position's draw."""

    def __init__(self, positions, n):
        self.positions, self.n_draws = list(positions), 0
        self.u = np.ones(n, dtype=np.float64)                # never read where no draw happened
        self.choice_at = np.full(n, 7, dtype=np.int32)       # likewise: a value the tests would notice
        self._random, self._choice = random.random, random.choice

    def __enter__(self):
        def rec_random():
            v = self._random()
            self.u[self.positions[self.n_draws]] = v
            self.n_draws += 1
            return v

        def rec_choice(seq):
            item = self._choice(seq)
            self.choice_at[self.positions[self.n_draws - 1]] = item[1]
            return item

        random.random, random.choice = rec_random, rec_choice
        return self

    def __exit__(self, *exc):
        random.random, random.choice = self._random, self._choice
        assert exc[0] is not None or self.n_draws == len(self.positions)
        return False


def main():
    from data.data_utils import merge_tokens, random_point_cloud, random_word
    tk = StubTokenizer()
    out = {}
    for L, Ls in C.SHAPES:
        inp = C.build_inputs(L, Ls)
        key = C.shape_key(L, Ls)
        for name, v in inp.items():
            out[f"{key}/{name}"] = v
        tok, off = inp["tok"], inp["off"]
        rows = [(C.text_of(tok, off, int(s)), C.text_of(tok, off, int(c))) for s, c in zip(inp["sent_idx"], inp["cap_idx"])]
        enc = [tk(s, L) for s, _ in rows]
        out[f"{key}/txt_ids"] = np.asarray([e[0] for e in enc], dtype=np.int64)
        out[f"{key}/txt_masks"] = np.asarray([e[1] for e in enc], dtype=np.int64)
        # the wrapper's string form: tokenizer(scene_cap + " " + sentence) (dataset_wrapper.py:49-54)
        enc_s = [tk(list(c) + list(s), Ls) for s, c in rows]
        out[f"{key}/scene_ids_str"] = np.asarray([e[0] for e in enc_s], dtype=np.int64)
        out[f"{key}/scene_masks_str"] = np.asarray([e[1] for e in enc_s], dtype=np.int64)
        # the pre-tokenised form (base.py:857-863); merge_tokens asserts len(token1) > len(token2), i.e. Ls > L
        if Ls > L:
            ids, masks = [], []
            for r, (s, c) in enumerate(rows):
                t1, m1 = tk(c, Ls)
                t2, m2 = tk(s, L)
                if r % 2:                                    # lists and tensors both reach it in the reference
                    t1, m1, t2, m2 = (torch.tensor(x) for x in (t1, m1, t2, m2))
                t1, m1 = merge_tokens(t1, m1, t2, m2, max_len=Ls, tokenizer=tk)
                ids.append(np.asarray(t1, dtype=np.int64))
                masks.append(np.asarray(m1, dtype=np.int64))
            out[f"{key}/scene_ids_merge"], out[f"{key}/scene_masks_merge"] = np.stack(ids), np.stack(masks)
        for ratio in C.RATIOS:
            rk = C.ratio_key(L, Ls, ratio)
            random.seed(7919 * L + Ls + int(ratio * 100))
            u_tok, rand_tok, ids, labels = [], [], [], []
            for e_ids, e_masks in enc:
                t_ids, t_masks = torch.tensor(e_ids), torch.tensor(e_masks)
                with Recorder(np.flatnonzero(e_masks), L) as rec:
                    o_ids, o_labels = random_word(t_ids, t_masks, tk, ratio)
                assert torch.equal(t_ids, torch.tensor(e_ids))                  # the input is left alone
                u_tok.append(rec.u), rand_tok.append(rec.choice_at)
                ids.append(o_ids.numpy()), labels.append(o_labels.numpy())
            u_obj, sem = [], []
            for row in inp["obj_masks"]:
                with Recorder(np.flatnonzero(row), len(row)) as rec:
                    sem.append(random_point_cloud([None] * len(row), torch.from_numpy(row), ratio).numpy())
                u_obj.append(rec.u)
            out[f"{rk}/u_tok"], out[f"{rk}/rand_tok"] = np.stack(u_tok), np.stack(rand_tok)
            out[f"{rk}/masked_ids"], out[f"{rk}/labels"] = np.stack(ids).astype(np.int64), np.stack(labels).astype(np.int64)
            out[f"{rk}/u_obj"], out[f"{rk}/obj_sem_masks"] = np.stack(u_obj), np.stack(sem)
            n_valid = int(out[f"{key}/txt_masks"].sum())
            print(f"{rk}: {n_valid} valid tokens, {(out[f'{rk}/labels'] != -1).sum()} masked, "
                  f"{(out[f'{rk}/rand_tok'] != 7).sum()} random replacements, objects kept "
                  f"{out[f'{rk}/obj_sem_masks'].sum()} of {inp['obj_masks'].sum()}")
    path = os.path.join(HERE, "text_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
