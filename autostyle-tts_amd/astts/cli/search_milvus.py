"""Restatement of /root/reference/src/search_milvus.py (:126-262): embed a query text and a speaker biography with the
Llama embedder, concatenate them into the 6144-d style-bank query, search the COSINE collection, print the hits.  Same
flags, same printed lines, same error convention (every stage prints + returns on failure; the search wrapper swallows to
[] -- :149-152).  The model is this build's GPU embedder (astts.llm.embedder.LlamaEmbedder) instead of an 8-bit PEFT
Llama under transformers (:36-72); a ready embedder can be injected (``main(args, embedder=...)``).

    python -m astts.cli.search_milvus --db_path milvus_demo.db --model_path /path/to/llama-3.2-3b \\
        --search_text "A man with a humorous style" --query_speaker ELIZABETH --top_k 3
"""
import argparse
import traceback

import numpy as np

from astts.compat.pymilvus import MilvusClient

# src/search_milvus.py:111-116
speaker_bio = {
    "ELIZABETH": "Elizabeth is a deeply emotional and passionate individual, extremely devoted to her husband Larry, willing to risk her life to hold onto their relationship.",
    "JOHN": "John is a pragmatic and thoughtful person, always considering the practical aspects of any situation. He values honesty and reliability in his relationships.",
    "PATRICIA": "Patricia is a thoughtful and reserved individual who values her privacy and independence. Her interactions reveal a sense of determination and a desire for meaningful connections.",
    "ANN": "Ann is a cheerful and optimistic person, always looking for the silver lining in every situation. She enjoys connecting with others and values strong interpersonal relationships.",
}


TOKENIZER_FILES = ("tokenizer.json", "tokenizer.model", "vocab.json", "tokenizer_config.json", "vocab.txt", "sentencepiece.bpe.model")


def load_tokenizer(model_path):
    """The checkpoint's own tokenizer when the directory has one and transformers can read it, else None (the caller then uses the hash
    stand-in).  The files are looked for first: for some model types (qwen2) AutoTokenizer builds an EMPTY tokenizer from config.json
    alone, without an error, and every text would encode to no tokens."""
    import os

    try:
        if not any(os.path.isfile(os.path.join(model_path, f)) for f in TOKENIZER_FILES):
            raise FileNotFoundError("none of " + ", ".join(TOKENIZER_FILES))
        from transformers import AutoTokenizer

        return AutoTokenizer.from_pretrained(model_path)
    except Exception as e:  # noqa: BLE001
        print(f"Warning: no tokenizer under '{model_path}' ({e}); using the hash stand-in")
        return None


def load_embedder(model_path, allow_random_init=False, seed=42, base_model_path=None, precision=None):
    """:36-72 ``load_model_and_tokenizer``: the checkpoint directory must exist (safetensors / .bin shards + tokenizer).
    A PEFT LoRA adapter directory (adapter_config.json: what the reference retrieves with) loads over its base checkpoint
    (``base_model_path``, else the adapter's base_model_name_or_path as a local directory or hub-cache snapshot; never fetched) and
    runs LLM.int8 + the unmerged LoRA branch, the reference's numerics; a merged checkpoint runs fp16.  ``precision`` ("int8" /
    "fp16") overrides either default.  The shape comes from the directory's config.json (Llama, Qwen2 or Qwen3; astts.llm.peft.shape_from_config).  Without a directory this raises unless random-init weights are explicitly allowed
    (plumbing runs, benchmarks).

    A directory whose config.json says model_type bert, roberta or xlm-roberta (m3e, bge, multilingual-e5; a sentence-transformers
    directory or a plain transformers one) is a sentence ENCODER and loads as an astts.llm.encoder_bert.BertEmbedder: the embedding calls
    of the class above, no generation; the other arguments do not apply to it."""
    import os

    from astts.llm.bert_dir import is_encoder_dir
    if model_path and os.path.isdir(model_path) and is_encoder_dir(model_path):      # another encoder family: refused there, by model_type
        return load_bert_embedder(model_path)

    from astts.llm.config import LlamaShape
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.peft import is_adapter_dir, load_peft_model, shape_from_config
    from astts.llm.weights import load_llama_weights, make_llama_weights

    cfg = LlamaShape.llama32_3b()
    if model_path and os.path.isdir(model_path):
        tok = load_tokenizer(model_path)
        if is_adapter_dir(model_path):
            if tok is not None and getattr(tok, "pad_token", None) is None and hasattr(tok, "eos_token"):
                tok.pad_token = tok.eos_token                                   # :47-48 of the reference: pad = eos
            state, cfg, adapter, _ = load_peft_model(model_path, base_model_path, len(tok) if tok is not None else None)
            int8 = (precision or "int8") == "int8"
            return LlamaEmbedder(state, cfg, tokenizer=tok, int8=int8, lora=adapter)
        state = load_llama_weights(model_path)
        if os.path.isfile(os.path.join(model_path, "config.json")):      # the checkpoint's own shape (Llama, Qwen2, Qwen3); else the 3.2-3B preset
            cfg = shape_from_config(model_path, int(state["model.embed_tokens.weight"].shape[0]))
        if (precision or "fp16") == "int8":
            return LlamaEmbedder(state, cfg, tokenizer=tok, int8=True)
        return LlamaEmbedder(state, cfg, tokenizer=tok)
    if not (allow_random_init or os.environ.get("ASTTS_ALLOW_RANDOM_INIT") == "1"):
        raise FileNotFoundError(f"no checkpoint directory at {model_path!r} (pass --allow_random_init to run on seeded random weights)")
    if os.environ.get("ASTTS_TINY_MODEL") == "1":
        cfg = LlamaShape.tiny()
    print(f"Warning: '{model_path}' not found; seeded RANDOM-INIT Llama weights at {cfg.hidden}-d (explicitly allowed)")
    return LlamaEmbedder(make_llama_weights(cfg, seed), cfg, int8=precision == "int8")


def load_bert_embedder(model_path):
    """A BERT-family encoder directory -> BertEmbedder: shape from config.json, pooling / normalisation / max_seq_length from the
    sentence-transformers files when present, the directory's own tokenizer (vocab.txt, tokenizer.json or sentencepiece.bpe.model)."""
    from astts.llm.bert_dir import bert_shape_from_config, sentence_setup
    from astts.llm.encoder_bert import BertEmbedder
    from astts.llm.weights import load_bert_weights

    shape = bert_shape_from_config(model_path)
    setup = sentence_setup(model_path, shape)
    return BertEmbedder(load_bert_weights(model_path, shape), shape, tokenizer=load_tokenizer(model_path), setup=setup)


def load_text_encoder(args):
    """``--embed_model_path DIR``: the model that embeds the texts in place of ``--model_path``'s LLM (which then only generates), or
    None without the flag."""
    path = getattr(args, "embed_model_path", "")
    return load_embedder(path) if path else None


# --embed_model_path of search_milvus, search_json and rag
EMBED_MODEL_HELP = ("directory of a sentence encoder (BERT / RoBERTa / XLM-R type: m3e, bge, multilingual-e5) that embeds the texts instead of "
                    "--model_path's LLM; labels and biographies are still generated by --model_path, and queries and the collection rag "
                    "creates are 2 x the encoder's hidden size wide")


def check_query_dim(client, collection_name, query_dim):
    """The query is 2 x the embedder's hidden size (6144 for Llama-3.2-3B, 7168 for Qwen2.5-7B, 1536 for m3e-base); a bank built with another model cannot
    be searched with it.  One message with both numbers instead of the search's byte count."""
    if not hasattr(client, "get_collection_info") or not client.has_collection(collection_name=collection_name):
        return                                  # a missing collection is reported where it is searched
    fields = client.get_collection_info(collection_name).get("fields", [])
    bank_dim = next((int(f["params"]["dim"]) for f in fields if "dim" in (f.get("params") or {})), None)
    if bank_dim is not None and bank_dim != int(query_dim):
        raise SystemExit(f"the query embedding has {int(query_dim)} dimensions (2 x the embedding model's hidden size {int(query_dim) // 2}) but collection "
                         f"'{collection_name}' holds {bank_dim}-dimensional vectors: this bank was built with another model")


def emb_text_bio(speaker, embedder):
    """:118-123"""
    return embedder.get_embedding(speaker_bio.get(speaker.upper(), "unknown"))


def search_milvus(client, collection_name, embedding, top_k=3):
    """:126-152"""
    try:
        return client.search(collection_name=collection_name, data=[embedding], anns_field="vector", metric_type="COSINE",
                             limit=top_k, output_fields=["file_id"])
    except Exception as e:  # noqa: BLE001
        print(f"Error during Milvus search: {e}")
        traceback.print_exc()
        return []


def main(args, embedder=None):
    encoder = load_text_encoder(args)            # this command only embeds: with --embed_model_path the LLM is not loaded at all
    if encoder is not None:
        embedder = encoder
    elif embedder is None:
        embedder = load_embedder(args.model_path, getattr(args, "allow_random_init", False), args.seed,
                                 getattr(args, "base_model_path", None), getattr(args, "llm_precision", None))
    try:
        client = MilvusClient(args.db_path)
        print(f"Connected to Milvus database at '{args.db_path}'.")
    except Exception as e:  # noqa: BLE001
        print(f"Error connecting to Milvus: {e}")
        traceback.print_exc()
        return None
    collection_name = args.collection_name
    if not client.has_collection(collection_name=collection_name):
        print(f"Collection '{collection_name}' does not exist. Please check the collection name.")
        return None
    try:
        collection_info = client.get_collection_info(collection_name)
        print(f"Collection '{collection_name}' info:")
        print(collection_info)
    except Exception as e:  # noqa: BLE001
        print(f"Error retrieving collection info: {e}")
        traceback.print_exc()
        return None
    check_query_dim(client, collection_name, 2 * embedder.cfg.hidden)
    query_text = args.search_text
    try:
        emotion_emb = embedder.get_embedding(query_text)                     # :214
        bio_emb = emb_text_bio(args.query_speaker, embedder)                 # :217
        combined_emb = np.concatenate((emotion_emb, bio_emb))                # :220
        combined_emb = combined_emb.astype(np.float32).tolist()
        print(f"Generated combined embedding of shape {len(combined_emb)}.")
    except Exception as e:  # noqa: BLE001
        print(f"Error generating embedding for the query text: {e}")
        traceback.print_exc()
        return None
    search_results = search_milvus(client, collection_name, combined_emb, top_k=args.top_k)
    if search_results:
        for query_idx, query_result in enumerate(search_results):
            print(f"\nTop {args.top_k} results for the query '{query_text}':")
            for res in query_result:
                print(f"File ID: {res['entity']['file_id']}, Distance: {res['distance']}")
            print("-" * 50)
    else:
        print("No results found.")
    return search_results


def build_parser():
    parser = argparse.ArgumentParser(description="Search embeddings in Milvus Lite")
    parser.add_argument("--db_path", type=str, default="milvus_demo.db", help="Path to the Milvus Lite database file")
    parser.add_argument("--collection_name", type=str, default="embeddings_biographies_collection",
                        help="Name of the Milvus collection to search")
    parser.add_argument("--model_path", type=str, default="",
                        help="Path to the fine-tuned Llama 3.2 model: a PEFT LoRA adapter directory (runs LLM.int8 + LoRA) or merged weights")
    parser.add_argument("--base_model_path", type=str, default=None, help="base checkpoint directory of a LoRA adapter (local only)")
    parser.add_argument("--embed_model_path", type=str, default="", help=EMBED_MODEL_HELP)
    parser.add_argument("--llm_precision", choices=("int8", "fp16"), default=None,
                        help="embedder weights: default int8 for an adapter directory, fp16 for merged weights")
    parser.add_argument("--allow_random_init", action="store_true",
                        help="run on seeded random weights when model_path does not exist (otherwise that is an error)")
    parser.add_argument("--search_text", type=str,
                        default="A man with a humorous style, from the countryside, with a very delicate mind",
                        help="Text to perform search in Milvus")
    parser.add_argument("--query_speaker", type=str, default="ELIZABETH", help="Speaker associated with the search text")
    parser.add_argument("--top_k", type=int, default=3, help="Number of top similar results to retrieve")
    parser.add_argument("--seed", type=int, default=42, help="Random seed for reproducibility")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
