"""Scoring a frontend checkpoint on the device, with the reference scripts' flags and printed lines:

    python -m wetts_amd.frontend_eval polyphone --polyphone_dict D --prosody_dict D --test_data F --checkpoint C \\
        --bert_name_or_path DIR [--batch_size 32] [--dtype f32|bf16|f16] # frontend/test_polyphone.py: "Accuracy: .."
    python -m wetts_amd.frontend_eval prosody   ... [--exclude_end]     # frontend/test_prosody.py: "pw f1_score .."
    python -m wetts_amd.frontend_eval cv --cv_polyphone_data F --cv_prosody_data F [--polyphone_weight 0.5] ...
                                                                        # the CV pass of frontend/train.py:43-94

--bert_name_or_path is a local directory with the BERT's `config.json` and `vocab.txt` (nothing is downloaded; its NAME
selects the transform layer's shape as in the reference).  The text is tokenised one token per character
(frontend_data.VocabTokenizer: equal to BERT's tokenisation for CJK characters only; for other text call
FrontendModel.score with frontend_data's classes and your own tokenizer).  One FrontendModel.score() call per batch;
what each call leaves (22 counts, two losses, the status word) stays on the device, the counts are added there, and
everything is read back ONCE at the end, so the CV lines (epoch 0, every batch) are printed after the last batch."""
import argparse
import os
import sys
from functools import partial

import torch

from .frontend import FrontendModel, HostScores, prosody_f1
from .frontend_data import FrontendDataset, VocabTokenizer, collate_fn, read_table


def get_args(argv=None):
    parser = argparse.ArgumentParser(prog="python -m wetts_amd.frontend_eval", description=__doc__.split("\n")[0])
    sub = parser.add_subparsers(dest="command", required=True)
    for name in ("cv", "polyphone", "prosody"):
        p = sub.add_parser(name)
        p.add_argument("--polyphone_dict", required=True, help="one pinyin per line; the line number is the class")
        p.add_argument("--prosody_dict", required=True, help="one prosody rank per line (#0 ..)")
        p.add_argument("--batch_size", type=int, default=32, help="sentences per score() call")
        p.add_argument("--checkpoint", required=True, help="the state_dict to score, as torch.save wrote it")
        p.add_argument("--bert_name_or_path", default="bert-chinese-base",
                       help="local directory holding the BERT's config.json and vocab.txt")
        p.add_argument("--dtype", choices=("f32", "bf16", "f16"), default="f32",
                       help="operands of the encoder's Linears (FrontendModel.set_dtype); f32 accumulation throughout")
        if name == "cv":
            p.add_argument("--cv_polyphone_data", required=True, help="polyphone lines of the validation set")
            p.add_argument("--cv_prosody_data", required=True, help="prosody lines of the validation set")
            p.add_argument("--polyphone_weight", type=float, default=0.5, help="w in loss = w * polyphone + (1 - w) * prosody")
        else:
            p.add_argument("--test_data", required=True, help="the lines to score")
        if name == "prosody":
            p.add_argument("--exclude_end", action="store_true", default=False,
                           help="leave each sentence's last break out of the F1 scores")
    return parser.parse_args(argv)


def _batches(data, batch_size, tokenizer):
    return torch.utils.data.DataLoader(data, batch_size=batch_size, shuffle=False,
                                       collate_fn=partial(collate_fn, tokenizer=tokenizer))


def run(args):
    """-> the printed lines (also printed)."""
    polyphone_dict, prosody_dict = read_table(args.polyphone_dict), read_table(args.prosody_dict)
    tokenizer = VocabTokenizer(os.path.join(args.bert_name_or_path, "vocab.txt"))
    if args.command == "cv":
        data = FrontendDataset(tokenizer, args.cv_polyphone_data, polyphone_dict, args.cv_prosody_data, prosody_dict)
    elif args.command == "polyphone":
        data = FrontendDataset(tokenizer, polyphone_file=args.test_data, polyphone_dict=polyphone_dict)
    else:
        data = FrontendDataset(tokenizer, prosody_file=args.test_data, prosody_dict=prosody_dict)
    model = FrontendModel(len(polyphone_dict), len(prosody_dict), os.path.join(args.bert_name_or_path, "config.json"),
                          bert_name_or_path=args.bert_name_or_path).set_dtype(getattr(args, "dtype", "f32"))
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True)).to("cuda")
    loader = _batches(data, args.batch_size, tokenizer)
    w = args.polyphone_weight if args.command == "cv" else 0.5
    rows = [model.score(inputs, phone_labels, prosody_labels, polyphone_weight=w).packed()
            for inputs, phone_labels, prosody_labels in loader]
    if not rows:
        raise SystemExit("no data")
    stacked = torch.stack(rows)
    # the counts are added on the device; they, every batch's row and its status word come back in ONE copy
    back = torch.cat([stacked[:, :22].sum(0), stacked.flatten()]).cpu()
    counts = back[:22].tolist()
    host = [HostScores.from_packed(r, w) for r in back[22:].reshape(len(rows), -1)]  # raises what a status word asks for
    lines = []
    if args.command == "polyphone":
        # test_polyphone.py:86 prints the quotient of two integer tensors, a float32
        lines.append("Accuracy: {}".format(torch.tensor(counts[1]) / torch.tensor(counts[0])))
    elif args.command == "prosody":
        lines.append("pw f1_score {} pph f1_score {} iph f1_score {}".format(*prosody_f1(counts, args.exclude_end)))
    else:
        for batch, h in enumerate(host):  # train.py:87-93 at its log interval of 1, epoch 0
            logstr = "Epoch {} [{}] progress {}/{} loss {:.6f}".format(0, "CV", batch, len(host), h.loss)
            logstr += " polyphone_loss {:.6f} polyphone_acc {:.6f}".format(h.phone_loss, h.phone_acc)
            logstr += " prosody_loss {:.6f} prosody_acc {:.6f}".format(h.prosody_loss, h.prosody_acc)
            lines.append(logstr)
    for line in lines:
        print(line)
    sys.stdout.flush()
    return lines


def main(argv=None):
    run(get_args(argv))


if __name__ == "__main__":
    main()
