"""A numpy model of the packed mlm rows over a byte-level BPE tokenizer in RoBERTa's form
(include/sdl_batcher.h "Packed mlm rows"): pack_model's stream over <s> ids </s> documents, then
mlm_policy_model's pick on every row as chunk 0 of record q -- id 0 a candidate, units from the "Ġ"
prefix, <pad> behind the flush row.  Also the RoBERTa-form tokenizer file the tests derive from the
gpt2 proxy.  A helper module, not a test."""
import json
import types

import numpy as np

import mlm_policy_model as M
import pack_model
from streaming_data_loader_amd import native

SEP, CLS, PAD, UNK, MASK = 50256, 50257, 50258, 50259, 50260


def roberta_tokenizer(path, pad=True, cls=CLS, mask_lstrip=False, post=True, keep_eot=False):
    """Writes the proxy in RoBERTa's form to `path`; -> its ids, vocabulary size and continuation flags."""
    with open(native.GPT2_PROXY_TOKENIZER, encoding="utf-8") as f:
        j = json.load(f)
    if not keep_eot:
        j["added_tokens"][0]["content"] = "</s>"
    for i, c in ((CLS, "<s>"), (PAD, "<pad>"), (UNK, "<unk>"), (MASK, "<mask>")):
        if pad or c != "<pad>":
            j["added_tokens"].append(dict(j["added_tokens"][0], id=i, content=c, lstrip=mask_lstrip and c == "<mask>"))
    if post:
        j["post_processor"] = {"type": "RobertaProcessing", "sep": ["</s>", SEP], "cls": ["<s>", cls],
                               "trim_offsets": True, "add_prefix_space": False}
    with open(path, "w", encoding="utf-8") as f:
        json.dump(j, f, ensure_ascii=False)
    cont = np.ones(MASK + 1, bool)  # cont = ~word_start: no "Ġ" prefix and no added token
    cont[[i for p, i in j["model"]["vocab"].items() if p.startswith("Ġ")] + [a["id"] for a in j["added_tokens"]]] = False
    return types.SimpleNamespace(path=str(path), cls=CLS, sep=SEP, pad=PAD, mask=MASK, vocab_size=MASK + 1, cont=cont)


def mask(ids, am, pos, ls, q0, tk, policy, seed, mask_length, per_mille=150):
    """Policy 1 / 2 over unmasked rows [G, S] with ls[g] filled positions -> the five planes [5, G, S]."""
    out, lab, S = ids.copy(), np.full_like(ids, -100), ids.shape[1]
    for g in range(ids.shape[0]):
        sel, _ = M.pick(ids[g], ls[g], M.row_words(seed, q0 + g, 0, S), policy, mask_length, per_mille,
                        {tk.cls, tk.sep, tk.mask, tk.pad}, tk.cont)
        u, rr = M.row_words(seed, q0 + g, M.DRAW_DOMAIN, S), M.row_words(seed, q0 + g, M.RANDOM_DOMAIN, S)
        for j in sel:
            lab[g, j] = ids[g, j]
            if int(u[j]) < M.MASK_BELOW:
                out[g, j] = tk.mask
            elif int(u[j]) < M.RANDOM_BELOW:
                out[g, j] = (int(rr[j]) * tk.vocab_size) >> 32
    return np.stack([out, am, np.zeros_like(ids), lab, pos])


def pack(id_lists, S, min_ids, carry, q0, tk, policy, seed, mask_length):
    """One call: -> ([5, G, S] planes: ids, attention, token types, labels, positions; new carry)."""
    docs = [[tk.cls] + list(t) for t in id_lists if len(t)]  # (pack_model keeps n + 2 >= min_ids of these)
    ids, am, _, pos, new_carry = pack_model.pack(docs, S, tk.sep, min_ids, carry)
    return mask(ids, am, pos, [S] * ids.shape[0], q0, tk, policy, seed, mask_length), new_carry


def flush(carry, S, q, tk, policy, seed, mask_length):
    """The flush row: [5, 0 or 1, S], the carry's c ids masked with l = c, <pad> behind them."""
    ids, am, _, pos = pack_model.flush(carry, S)
    ids[:, len(carry[0]):] = tk.pad
    return mask(ids, am, pos, [len(carry[0])] * ids.shape[0], q, tk, policy, seed, mask_length)
