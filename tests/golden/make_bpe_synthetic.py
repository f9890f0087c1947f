"""A synthetic BPE merges file in the format of CLIP's bpe_simple_vocab_16e6.txt.gz, so that the
tokenizer tests need no file from outside the repository: one header line, then 48,894 merges
"a b" over byte-level symbols (the GPT-2 byte -> printable-character map; a word's last symbol
carries "</w>").  The merges are learnt here by plain BPE on a small corpus written for this purpose
(so that they fire on the test texts), then filled up to the real file's used length with seeded
random pairs of byte symbols, which keeps the vocabulary at CLIP's 49,408 entries.

    python tests/golden/make_bpe_synthetic.py        # writes tests/golden/bpe_synthetic.txt.gz

tests/golden/make_golden_tokenizer.py --synthetic then records what the reference's tokenizer makes
of the test texts with this file (tests/golden/tokenizer_synthetic.npz)."""
import collections
import gzip
import os
import random
import re

HERE = os.path.dirname(os.path.abspath(__file__))
N_MERGES = 49152 - 256 - 2

CORPUS = """
a photo of a cat . a photo of a dog . a picture of the table and the laptop . the cat is to the left
of a tree and the dog is to the right of the tree . a mug on top of a table , a mug under a table ,
a bowl in front of a laptop , a bowl behind a laptop . is the butterfly's wing visible ? the cat's
toy isn't here ; we'll see , they've gone , i'm sure , you'd go , we're ok . she'll go , it's , they'd .
rock'n'roll quoted single . 1234 apples and 56.78 kg at 09:30 . leading and trailing spaces tabs newline .
hello world foo bar baz qux quux . café naïve résumé ångström decomposed acute . emoji mixed long ligature
straße zero width nbsp here ideographic sep html amp quot start of text end of text literal specials upper
curly apostrophe don't under score snake case dash slash back . a very long caption word word1 word2 word3
word10 word20 word99 word100 word119 . supercalifragilisticexpialidocious antidisestablishmentarianism .
the photo shows two red apples and a green pear on a wooden table next to a window . three blue birds
over the river near an old stone bridge , four white horses running through tall yellow grass , people
walking along the street with umbrellas in the rain , children playing football in the park at sunset .
москва столица россии привет мир . 北京 的 天安门 广场 你好 世界 . مرحبا بالعالم .
"""


def bytes_to_unicode():
    """The GPT-2 map: printable Latin-1 bytes stand for themselves, the others for U+0100 upwards."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def learn(words, limit):
    """Plain BPE: merge the most frequent adjacent pair (ties: the smaller pair) until none occurs twice."""
    merges = []
    while len(merges) < limit:
        pairs = collections.Counter()
        for w, c in words.items():
            for p in zip(w, w[1:]):
                pairs[p] += c
        if not pairs:
            break
        best = min(pairs, key=lambda p: (-pairs[p], p))
        if pairs[best] < 2:
            break
        merges.append(best)
        new = {}
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1])
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            new[tuple(out)] = new.get(tuple(out), 0) + c
        words = new
    return merges


def main():
    enc = bytes_to_unicode()
    words = collections.Counter()
    for tok in re.findall(r"[^\W\d_]+|\d|[^\s\w]+|_", CORPUS.lower()):
        s = [enc[b] for b in tok.encode("utf-8")]
        s[-1] += "</w>"
        words[tuple(s)] += 1
    # every merge names a new vocabulary entry a + b: keep the first of any that spell the same one
    merges, seen = [], set()
    for a, b in learn(dict(words), N_MERGES):
        if a + b not in seen:
            seen.add(a + b)
            merges.append((a, b))
    learnt = len(merges)
    rng = random.Random(20240607)
    syms = sorted(enc.values())
    while len(merges) < N_MERGES:
        a, b = rng.choice(syms), rng.choice(syms) + ("</w>" if rng.random() < 0.25 else "")
        if a + b not in seen:
            seen.add(a + b)
            merges.append((a, b))
    text = '"synthetic merges for the tokenizer tests (tests/golden/make_bpe_synthetic.py)"\n'
    text += "".join(f"{a} {b}\n" for a, b in merges)
    path = os.path.join(HERE, "bpe_synthetic.txt.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(text.encode("utf-8"))
    print(f"wrote {path}: {learnt} learnt + {N_MERGES - learnt} filler merges, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
