"""A byte-level tokenizer for the evaluation tests (no tokenizer files exist offline): bos + one id per UTF-8 byte, the two ChatML
markers as single special ids.  Fits LlamaShape.tiny() (vocab 512, bos 1, eos 2).  Reversible, unlike astts' HashTokenizer, so that
``post_process`` sees real text."""

BOS, EOS, IM_START, IM_END = 1, 2, 300, 301
SPECIAL = {IM_START: "<|im_start|>", IM_END: "<|im_end|>", BOS: "<|begin_of_text|>", EOS: "<|end_of_text|>"}


class ByteTokenizer:
    chat_template = None
    eos_token_id, pad_token_id = EOS, EOS

    def encode(self, text, add_special_tokens=True):
        ids = [BOS] if add_special_tokens else []
        i = 0
        while i < len(text):
            for tid in (IM_START, IM_END):
                if text.startswith(SPECIAL[tid], i):
                    ids.append(tid)
                    i += len(SPECIAL[tid])
                    break
            else:
                ids.extend(3 + b for b in text[i].encode("utf-8"))
                i += 1
        return ids

    def decode(self, ids, skip_special_tokens=False):
        out, buf = [], bytearray()
        for t in ids:
            t = int(t)
            if 3 <= t < 259:
                buf.append(t - 3)
                continue
            out.append(buf.decode("utf-8", "replace"))
            buf = bytearray()
            if not skip_special_tokens:
                out.append(SPECIAL.get(t, f"<{t}>"))
        out.append(buf.decode("utf-8", "replace"))
        return "".join(out)
