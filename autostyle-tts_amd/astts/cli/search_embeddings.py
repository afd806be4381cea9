"""Restatement of /root/reference/milvus/search_embeddings.py: same flags, same printed lines, same error
convention (the wrapper swallows search errors: print + traceback, return [] -- :24-27), served by the HBM-resident
style bank through the MilvusClient shim.

    python -m astts.cli.search_embeddings --query_embedding q.json --top_k 3 --db_path milvus_demo.db
Beyond the reference: ``--group_by_field FIELD [--group_size N]`` returns the top_k closest groups of FIELD, N hits of each;
``--use_index [--nlist N] [--nprobe P]`` searches through an IVF_FLAT index of N lists (default: the collection's own request, else
128), probing P of them (default 10, the reference's ``param``) -- without it the search is the exact brute-force one.
"""
import argparse
import json
import traceback

from astts.compat.pymilvus import MilvusClient


def search_milvus(client, collection_name, embedding, top_k=3, group_by_field=None, group_size=1, nprobe=10):
    try:
        param = {"nprobe": nprobe}
        grouping = {"group_by_field": group_by_field, "group_size": group_size} if group_by_field else {}
        return client.search(collection_name=collection_name, data=[embedding], anns_field="vector", param=param,
                             limit=top_k, output_fields=["file_id", "text"], **grouping)
    except Exception as e:  # noqa: BLE001 -- the reference degrades to [] on any failure
        print(f"Error during Milvus search: {e}")
        traceback.print_exc()
        return []


def main(args):
    name = "embeddings_biographies_collection"
    client = MilvusClient(args.db_path, use_index=args.use_index)
    if args.use_index and client.has_collection(name) and (args.nlist is not None or client._get(name).ivf_nlist() is None):
        client.create_index(name, "vector", {"index_type": "IVF_FLAT", "params": {"nlist": args.nlist if args.nlist is not None else 128}})
    print(f"Connected to Milvus at '{args.db_path}'.")
    try:
        with open(args.query_embedding, "r", encoding="utf-8") as f:
            query_embedding = json.load(f)
        print(f"Loaded query embedding from '{args.query_embedding}'.")
    except Exception as e:  # noqa: BLE001
        print(f"Error loading query embedding: {e}")
        traceback.print_exc()
        return []
    search_results = search_milvus(client, name, query_embedding, top_k=args.top_k,
                                   group_by_field=args.group_by_field, group_size=args.group_size, nprobe=args.nprobe)
    if search_results:
        for i, result in enumerate(search_results):
            print(f"\nTop {args.top_k} results for Query {i + 1}:")
            for res in result:
                if args.group_by_field:      # (top_k groups of up to group_size hits, in the order of their best hits)
                    print(f"Group {args.group_by_field}={res['entity'].get(args.group_by_field)!r}: ", end="")
                print(f"File ID: {res['entity']['file_id']}, Distance: {res['distance']}, Text: {res['entity']['text']}")
            print("-" * 50)
    else:
        print("No results found.")
    return search_results


def build_parser():
    parser = argparse.ArgumentParser(description="Search embeddings in Milvus Lite")
    parser.add_argument("--query_embedding", type=str, required=True,
                        help="Path to the JSON file containing the query embedding vector")
    parser.add_argument("--top_k", type=int, default=3, help="Number of top similar results to retrieve")
    parser.add_argument("--db_path", type=str, default="milvus_demo.db", help="Path to the Milvus Lite database file")
    # not in the reference: grouped search of the style bank (off by default: output as the reference prints it)
    parser.add_argument("--group_by_field", type=str, default=None,
                        help="Return the top_k closest GROUPS of this scalar field (or the primary key) instead of the top_k hits")
    parser.add_argument("--group_size", type=int, default=1, help="Hits per group (with --group_by_field)")
    # not in the reference: the IVF_FLAT index (off by default: every search is exact)
    parser.add_argument("--use_index", action="store_true", help="Search through an IVF_FLAT index instead of the exact scan")
    parser.add_argument("--nlist", type=int, default=None, help="Lists of the index (with --use_index; default: the collection's, else 128)")
    parser.add_argument("--nprobe", type=int, default=10, help="Lists probed per query (with --use_index)")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
