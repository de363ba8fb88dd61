"""The frontend's training / evaluation data as the reference reads it (frontend/dataset.py:19-154, frontend/utils.py):
IGNORE_ID, read_table, FrontendDataset and collate_fn with its line formats and label placement, for any tokenizer that
offers `encode(text, add_special_tokens=False)` and the batch call
`tokenizer(list of word lists, padding=True, truncation=True, is_split_into_words=True, return_tensors="pt")`
(a Hugging Face tokenizer does), and VocabTokenizer, a `transformers`-free one for Chinese text.

Line formats.  Polyphone data: a polyphone's pinyin follows its character between two `▁` marks
(`宋代出现了▁le5▁燕乐音阶的记载`); the label sits at the LAST token of the text before the mark, a pinyin that the dict does
not list leaves it ignored.  Prosody data: `word #N` pairs (`今天 #1 天气 #1 怎么样 #3`); every token is labelled 0 except a
word's last one, which carries N; a line with an odd number of fields, a rank that is not `#digits` or a rank >=
len(prosody_dict) is skipped with "Ignore line ..".  collate_fn writes a sample's labels at the positions 1 .. len (position
0 is [CLS]) and IGNORE_ID everywhere else.  parse_polyphone_line / parse_prosody_line are the two formats on their own,
without a tokenizer."""
import numpy as np
import torch

IGNORE_ID = -100


def read_table(fname):
    """frontend/utils.py: one name per line -> {name: line number}."""
    table = {}
    with open(fname, encoding="utf8") as fin:
        for i, line in enumerate(fin):
            table[line.strip()] = i
    return table


class VocabTokenizer:
    """One token per character from a BERT `vocab.txt`; a character the vocabulary does not list becomes [UNK]; whitespace
    separates and is dropped.  This EQUALS BERT's tokenisation (BasicTokenizer + WordPiece) for CJK characters only, which
    BERT always splits one by one: a run of Latin letters or digits is one or several WordPiece tokens there and one
    token PER CHARACTER here.  For such text pass your own Hugging Face tokenizer to FrontendDataset / collate_fn."""

    def __init__(self, vocab_file, model_max_length=None):
        self.vocab = read_table(vocab_file)
        for t in ("[PAD]", "[UNK]", "[CLS]", "[SEP]"):
            if t not in self.vocab:
                raise ValueError(f"{vocab_file} has no {t} token")
        self.pad_token_id, self.unk_token_id = self.vocab["[PAD]"], self.vocab["[UNK]"]
        self.cls_token_id, self.sep_token_id = self.vocab["[CLS]"], self.vocab["[SEP]"]
        self.model_max_length = model_max_length

    def encode(self, text, add_special_tokens=False):
        ids = [self.vocab.get(ch, self.unk_token_id) for ch in text if not ch.isspace()]
        return [self.cls_token_id] + ids + [self.sep_token_id] if add_special_tokens else ids

    def __call__(self, batch_sentence, padding=True, truncation=True, is_split_into_words=True, return_tensors="pt"):
        if not (padding is True and is_split_into_words and return_tensors == "pt"):
            raise ValueError("VocabTokenizer serves collate_fn's call only: padding=True, is_split_into_words=True, "
                             "return_tensors='pt'")
        rows = []
        for words in batch_sentence:
            ids = [i for w in words for i in self.encode(w)]
            if truncation and self.model_max_length is not None:
                ids = ids[:self.model_max_length - 2]
            rows.append([self.cls_token_id] + ids + [self.sep_token_id])
        T = max(len(r) for r in rows)
        input_ids = torch.full((len(rows), T), self.pad_token_id, dtype=torch.int64)
        mask = torch.zeros(len(rows), T, dtype=torch.int64)
        for b, r in enumerate(rows):
            input_ids[b, :len(r)] = torch.tensor(r, dtype=torch.int64)
            mask[b, :len(r)] = 1
        return {"input_ids": input_ids, "token_type_ids": torch.zeros_like(input_ids), "attention_mask": mask}


MARK = "\u2581"  # the polyphone files' mark around a pinyin
_DIGITS = frozenset("0123456789")


def parse_polyphone_line(line):
    """One line of a polyphone file -> [(text piece, pinyin or None), ..]: the fields between the marks alternate between
    text and the pinyin of the text's last character; marks at either end of the line carry nothing."""
    fields = line.strip().strip(MARK).split(MARK)
    return [(text, fields[k + 1] if k + 1 < len(fields) else None) for k, text in list(enumerate(fields))[::2]]


def parse_prosody_line(line, num_ranks):
    """One line of a prosody file -> [(word, rank), ..], or None for a line that is not a sequence of `word #N` pairs
    with N a run of ASCII digits below num_ranks."""
    fields = line.split()
    if len(fields) % 2:
        return None
    pairs = []
    for word, mark in zip(fields[::2], fields[1::2]):
        number = mark[1:]
        if mark[0] != "#" or not number or not set(number) <= _DIGITS or int(number) >= num_ranks:
            return None
        pairs.append((word, int(number)))
    return pairs


class FrontendDataset(torch.utils.data.Dataset):
    """The samples the reference's FrontendDataset holds, {"sentence": [text pieces], "polyphones": [label per token],
    "prosody": [label per token]}: the polyphone file's lines first, then the prosody file's.  A file is read only where
    its dict is given too.  Prints the reference's two kinds of log line."""

    def __init__(self, tokenizer=None, polyphone_file=None, polyphone_dict=None, prosody_file=None, prosody_dict=None):
        self.tokenizer = tokenizer
        self.polyphone_dict, self.prosody_dict = polyphone_dict, prosody_dict
        self.data = []
        for kind, fname, table, reader in (("polyphone", polyphone_file, polyphone_dict, self.read_polyphone_data),
                                           ("prosody", prosody_file, prosody_dict, self.read_prosody_data)):
            if fname is not None and table is not None:
                samples = reader(fname)
                print("Reading {} {} data".format(len(samples), kind))
                self.data.extend(samples)

    def _count(self, text):
        return len(self.tokenizer.encode(text, add_special_tokens=False))

    def read_polyphone_data(self, polyphone_file):
        """The label of a marked character sits on the LAST token of its piece; a pinyin outside the dict stays ignored."""
        samples = []
        with open(polyphone_file, encoding="utf8") as f:
            for line in f:
                pieces = parse_polyphone_line(line)
                labels = []
                for text, pinyin in pieces:
                    n = self._count(text)
                    labels += [IGNORE_ID] * n
                    if n and pinyin is not None and pinyin in self.polyphone_dict:
                        labels[-1] = self.polyphone_dict[pinyin]
                samples.append({"sentence": [text for text, _ in pieces], "polyphones": labels,
                                "prosody": [IGNORE_ID] * len(labels)})
        return samples

    def read_prosody_data(self, prosody_file):
        """Every token is labelled 0 except a word's last one, which carries the word's rank."""
        samples = []
        with open(prosody_file, encoding="utf8") as f:
            for line in f:
                pairs = parse_prosody_line(line, len(self.prosody_dict))
                if pairs is None:
                    print("Ignore line {}".format(line.strip()))
                    continue
                labels = []
                for word, rank in pairs:
                    n = self._count(word)
                    labels += [0] * n
                    if n:
                        labels[-1] = rank
                samples.append({"sentence": [word for word, _ in pairs], "polyphones": [IGNORE_ID] * len(labels),
                                "prosody": labels})
        return samples

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        return self.data[idx]


def collate_fn(batch_samples, tokenizer):
    """dataset.py:129-154 -> (inputs dict, polyphone labels [B, T], prosody labels [B, T]) int64."""
    batch_inputs = tokenizer([s["sentence"] for s in batch_samples], padding=True, truncation=True,
                             is_split_into_words=True, return_tensors="pt")
    shape = tuple(batch_inputs["input_ids"].shape)
    polyphone_label = np.full(shape, IGNORE_ID, dtype=np.int64)
    prosody_label = np.full(shape, IGNORE_ID, dtype=np.int64)
    for idx, s in enumerate(batch_samples):
        polyphone_label[idx][1:len(s["polyphones"]) + 1] = np.array(s["polyphones"], dtype=np.int64)
        prosody_label[idx][1:len(s["prosody"]) + 1] = np.array(s["prosody"], dtype=np.int64)
    return batch_inputs, torch.tensor(polyphone_label), torch.tensor(prosody_label)
