"""Style-bank construction: /root/reference/milvus/RAG.py (:400-621) on one GPU in one command.

    python -m astts.cli.rag --model_path /path/to/llama-3.2-3b --data_folder talk1.json talk2.json --db_path milvus_demo.db \
        --output_file embeddings_biographies.json [--search_text "..."] [--top_k 3]

Utterances {speaker, zh_text, file_id} (JSON lists or JSONL; a directory contributes its *.json: :269-331) are grouped by speaker
(:334-356); each speaker gets ONE sampled biography from its utterances joined with "\n" (:484-487: do_sample=True, temperature 0.7,
top_p 0.9, --max_new_tokens), each utterance a greedy emotion label (:495), and [label embedding | biography embedding] (:498) goes
into a fresh ``embeddings_biographies_collection`` of dimension 2 * hidden as {id, file_id, vector, text} with the primary key
restarting at 1 for every speaker, as :507 does.  The JSON dump (:514-521, :560-561), the self-retrieval check (:568-582, the same line
per query) and the ``--search_text`` query (:585-617) follow.  The file is a Milvus-Lite database: ``MilvusClient(db_path)``,
astts.cli.search_json and astts.cli.search_embeddings open it unchanged.

Batched where the reference loops: ``--llm_batch`` speakers per sampled decode and utterances per greedy decode, every DISTINCT label /
biography text embedded once (astts.cli.search_json.embed_rows), all self-retrieval queries in one search.  Every token of a biography
is drawn on the GPU (astts_op_sample_topk_topp); the draws are keyed by ``--seed`` and the speaker's place among the speakers, so the
same command writes the same files.

Not taken over: the output-file-name derivation of :425-452 (``--output_file`` is used as given; empty: no dump).  A speaker whose
biography cannot be generated gets the placeholder text of milvus/search_json.py:378 instead of being dropped, and the
``--search_text`` query reuses the first speaker's biography instead of sampling a second one for the same speaker (:595).
"""
import argparse
import json
import os
import traceback
from glob import glob

import numpy as np

from astts.cli.search_json import embed_rows, generate_speaker_biographies
from astts.cli.search_milvus import EMBED_MODEL_HELP
from astts.compat.pymilvus import MilvusClient

COLLECTION = "embeddings_biographies_collection"          # RAG.py:457
FIELDS = ("speaker", "zh_text", "file_id")


def load_all_json_files(paths):
    """RAG.py:269-331: files and the *.json of directories; a JSON list or JSONL; objects without all of FIELDS are skipped."""
    files = []
    for p in paths:
        if os.path.isfile(p):
            files.append(p)
        elif os.path.isdir(p):
            files.extend(sorted(glob(os.path.join(p, "*.json"))))
        else:
            print(f"Invalid data path: {p}")
    data = []
    for path in files:
        loaded = skipped = 0
        try:
            with open(path, "r", encoding="utf-8") as f:
                text = f.read()
            if text[:1] == "[":
                items = json.loads(text)
                if not isinstance(items, list):
                    print(f"Unsupported JSON structure in file {path}.")
                    items = []
            else:
                items = []
                for n, line in enumerate(text.splitlines(), 1):
                    if line.strip():
                        try:
                            items.append(json.loads(line))
                        except json.JSONDecodeError as e:
                            print(f"JSON decode error in file {path} at line {n}: {e}")
            for it in items:
                if not isinstance(it, dict):
                    print(f"Unsupported item format in file {path}.")
                elif all(k in it for k in FIELDS):
                    data.append(it)
                    loaded += 1
                else:
                    skipped += 1
        except Exception as e:  # noqa: BLE001
            print(f"Error loading file {path}: {e}")
            traceback.print_exc()
            continue
        print(f"Loaded {loaded} samples from '{path}'. Skipped {skipped} samples due to missing fields.")
    return data


def group_by_speaker(data):
    """RAG.py:334-356: {speaker: [{file_id, text}]}; samples without text or file_id are skipped."""
    out = {}
    for s in data:
        text, fid = s.get("zh_text", "").strip(), s.get("file_id", None)
        if text and fid:
            out.setdefault(s.get("speaker", "UNKNOWN_SPEAKER"), []).append({"file_id": fid, "text": text})
    return out


def main(args, client=None, embedder=None):
    data = load_all_json_files(args.data_folder)
    print(f"Loaded {len(data)} samples from '{args.data_folder}'.")
    if not data:
        print("No data loaded. Please check the data format and path.")
        return None
    speakers = group_by_speaker(data)
    print(f"Found {len(speakers)} unique speakers.")
    if not speakers:
        print("No speakers found. Please check the data contents.")
        return None
    if embedder is None:
        from astts.cli.search_milvus import load_embedder
        embedder = load_embedder(args.model_path, getattr(args, "allow_random_init", False), args.seed, getattr(args, "base_model_path", None),
                                 getattr(args, "llm_precision", None))
    from astts.cli.search_milvus import load_text_encoder
    encoder = load_text_encoder(args) or embedder        # --embed_model_path: the sentence encoder embeds, the LLM only generates
    dim = 2 * encoder.cfg.hidden                                                                    # :458
    client = client or MilvusClient(args.db_path)
    if client.has_collection(collection_name=COLLECTION):                                           # :49-51
        client.drop_collection(collection_name=COLLECTION)
        print(f"Existing collection '{COLLECTION}' dropped.")
    client.create_collection(collection_name=COLLECTION, dimension=dim)
    print(f"Collection '{COLLECTION}' created successfully with quick setup.")

    batch = getattr(args, "llm_batch", 32)
    conv = {s: "\n".join(u["text"] for u in utts) for s, utts in speakers.items()}               # :484
    bios = generate_speaker_biographies(conv, embedder, args.max_new_tokens, batch, args.seed)
    flat = [{"speaker": s, "zh_text": u["text"], "file_id": u["file_id"], "pk": i + 1} for s, utts in speakers.items() for i, u in enumerate(utts)]
    q, labels, failed = embed_rows(flat, embedder, bios, max_new_tokens=10, batch=batch, encoder=encoder)
    results, insert = [], []
    for r, vec, lab, bad in zip(flat, q, labels, failed):
        if bad:
            print(f"Error processing speaker {r['speaker']}: no embedding for file {r['file_id']}")
            continue
        insert.append({"id": r["pk"], "file_id": r["file_id"], "vector": vec.tolist(), "text": r["zh_text"]})      # :506-511
        results.append({"file_id": r["file_id"], "speaker": r["speaker"], "text": r["zh_text"], "emotion": lab, "biography": bios[r["speaker"]],
                        "combined_embedding_shape": [int(vec.shape[0])]})
        if getattr(args, "verbose", False):
            print(f"File ID: {r['file_id']}\nSpeaker: {r['speaker']}\nText: {r['zh_text']}\nEmotion: {lab}\nBiography: {bios[r['speaker']]}\n"
                  f"Combined Embedding Shape: {vec.shape}\n" + "=" * 50)
    if insert:
        client.insert(collection_name=COLLECTION, data=insert)
        print("Combined embeddings inserted successfully.")
    else:
        print("No data to insert into Milvus.")
    if args.output_file:
        out_dir = os.path.dirname(args.output_file)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
        with open(args.output_file, "w", encoding="utf-8") as f:
            json.dump(results, f, ensure_ascii=False, indent=2)
        print(f"Embeddings and biographies saved to '{args.output_file}'.")
    verify = []
    if insert:                                                                                       # :568-582, one search for all queries
        print("\nVerifying inserted embeddings by searching with inserted vectors:")
        verify = client.search(collection_name=COLLECTION, data=np.asarray([it["vector"] for it in insert], np.float32), limit=1, filter=None,
                               output_fields=["file_id", "text"])
        for i, hits in enumerate(verify):
            for res in hits:
                ent = res.get("entity", {})
                print(f"Query ID: {i + 1}, Retrieved ID: {res.get('id')}, Distance: {res.get('distance')}, File ID: {ent.get('file_id')}, "
                      f"Text: {ent.get('text')}")
            if not hits:
                print(f"No results found for Query ID: {i}")
    found = None
    if args.search_text and insert:                                                                  # :585-617
        print(f"\nPerforming search for the input text: '{args.search_text}'")
        try:
            first = next(iter(speakers))
            sq, slab, sbad = embed_rows([{"zh_text": args.search_text, "speaker": first}], embedder, bios, max_new_tokens=10, batch=1, encoder=encoder)
            if sbad[0]:
                raise RuntimeError("no embedding for the search text")
            found = client.search(collection_name=COLLECTION, data=sq, limit=args.top_k, filter=None, output_fields=["file_id", "text"])
            for hits in found:
                print(f"\nTop {args.top_k} results for the query '{args.search_text}':")
                for res in hits:
                    ent = res.get("entity", {})
                    print(f"File ID: {ent.get('file_id')}, Distance: {res.get('distance')}, Text: {ent.get('text')}")
                print("-" * 50)
        except Exception as e:  # noqa: BLE001
            print(f"Error during search: {e}")
            traceback.print_exc()
    return {"results": results, "inserted": insert, "biographies": bios, "verify": verify, "search": found}


def build_parser():
    p = argparse.ArgumentParser(description="Generate emotion and biography embeddings and store them in Milvus Lite")
    p.add_argument("--model_path", type=str, default="", help="Llama-3.2-3B directory: a PEFT LoRA adapter (LLM.int8 + LoRA, as the reference) "
                   "or merged weights + tokenizer")
    p.add_argument("--base_model_path", default=None, help="base checkpoint directory of a LoRA adapter (local only; nothing is fetched)")
    p.add_argument("--embed_model_path", default="", help=EMBED_MODEL_HELP)
    p.add_argument("--llm_precision", choices=("int8", "fp16"), default=None,
                   help="embedder weights: default int8 for an adapter directory, fp16 for merged weights")
    p.add_argument("--allow_random_init", action="store_true", help="run on seeded random Llama weights when model_path does not exist")
    p.add_argument("--llm_batch", type=int, default=32, help="speakers per sampled decode, utterances per greedy decode / embedding pass")
    p.add_argument("--data_folder", type=str, nargs="+", required=True, help="JSON / JSONL files, or folders of *.json, of {speaker, zh_text, file_id}")
    p.add_argument("--output_file", type=str, default="", help="JSON dump of the utterances with emotion and biography (used as given)")
    p.add_argument("--db_path", type=str, default="milvus_demo.db", help="Path to the Milvus Lite database file")
    p.add_argument("--seed", type=int, default=42, help="Random seed for reproducibility")
    p.add_argument("--max_new_tokens", type=int, default=250, help="Maximum number of new tokens to generate for a biography")
    p.add_argument("--search_text", type=str, default="A man with a humorous style, from the countryside, with a very delicate mind",
                   help="Text to perform search in Milvus (empty: none)")
    p.add_argument("--top_k", type=int, default=3, help="Number of top similar results to retrieve")
    p.add_argument("--verbose", action="store_true", help="print every utterance's record, as the reference does")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
