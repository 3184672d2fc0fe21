//go:build mi355x

// The MI355X build's batch form of ImmuStore.DualProof (immustore.go:2394-2463,
// with LinearProof :2472-2510 and LinearAdvanceProof :2514-2562) followed by
// DualProofToProto + Marshal (pkg/api/schema/database_protoconv.go:131-211):
// the answers of a batch of VerifiableGet / VerifiableSet / VerifiableTxById
// requests (pkg/database/database.go:805,881) generated and encoded in one
// device pass over a dLog kept resident beside the store's aht, instead of one
// walk over the tree and the tx log per proof.  Uncompiled in the build image
// (no Go toolchain); see go/README.md.
package store

/*
#cgo CFLAGS: -I${SRCDIR}/../../third_party/immustore_amd/include
#cgo LDFLAGS: -L${SRCDIR}/../../third_party/immustore_amd -limmustore_merkle -Wl,-rpath,${SRCDIR}/../../third_party/immustore_amd
#include <stdlib.h>
#include "immustore_merkle.h"
*/
import "C"

import (
	"crypto/sha256"
	"encoding/binary"
	"math"
	"runtime"
	"unsafe"

	"github.com/codenotary/immudb/embedded/internal/mi355x"
)

// ProofTree is the store's aht mirrored on the device: the caller appends the
// same Alh values the store appends to s.aht (immustore.go:1198-1232,
// :1764-1770), in the same order.
type ProofTree struct {
	t *C.mh_ahtree
}

func NewProofTree() (*ProofTree, error) {
	p, err := mi355x.Context()
	if err != nil {
		return nil, err
	}
	pt := &ProofTree{}
	if st := C.mh_ahtree_new((*C.mh_ctx)(p), &pt.t); st != C.MH_OK {
		return nil, mapErr(st)
	}
	runtime.SetFinalizer(pt, func(pt *ProofTree) { C.mh_ahtree_free(pt.t) })
	return pt, nil
}

// AppendBatch appends the Alh of every tx of a run, as aht.Append(alh[:]) does
// one.
func (pt *ProofTree) AppendBatch(alhs [][sha256.Size]byte) error {
	if len(alhs) == 0 {
		return nil
	}
	return mapErr(C.mh_ahtree_append_batch(pt.t, (*C.uint8_t)(unsafe.Pointer(&alhs[0][0])),
		C.uint64_t(len(alhs)), C.uint32_t(sha256.Size), nil))
}

// mapProofErr: DualProof's own sentinel beside the store-wide mapping.
func mapProofErr(st C.int) error {
	if st == C.MH_ERR_SOURCE_TX_NEWER {
		return ErrSourceTxNewerThanTargetTx // immustore.go:101
	}
	return mapErr(st)
}

func packHeaders(hdrs []*TxHeader, blob *[]byte) []C.mh_tx_header {
	out := make([]C.mh_tx_header, len(hdrs)+1)
	for i, h := range hdrs {
		o := &out[i]
		o.id, o.ts, o.bl_tx_id = C.uint64_t(h.ID), C.int64_t(h.Ts), C.uint64_t(h.BlTxID)
		o.version, o.nentries = C.uint32_t(h.Version), C.uint32_t(h.NEntries)
		for k := 0; k < sha256.Size; k++ {
			o.bl_root[k], o.prev_alh[k], o.eh[k] = C.uint8_t(h.BlRoot[k]), C.uint8_t(h.PrevAlh[k]), C.uint8_t(h.Eh[k])
		}
		if h.Metadata != nil { // tx.go:483-501: nil when the stored length is 0
			md := h.Metadata.Bytes()
			o.md_off, o.md_len = C.uint32_t(len(*blob)), C.uint32_t(len(md))
			*blob = append(*blob, md...)
		}
	}
	return out
}

// DualProofBatch is ImmuStore.DualProof(src[p], tgt[p]) marshalled as
// schema.DualProof, for every pair.  alh / inner are the digest window: Alh()
// and innerHash() of the txs firstTx .. firstTx + len(alh) - 1 (the linear
// parts are runs of them; the tree holds only SHA-256(0x00 || Alh)).  msgs[p]
// is the message, or nil with errs[p] the error DualProof would have returned:
// ErrIllegalArguments, ErrSourceTxNewerThanTargetTx, ErrCorruptedTxData,
// ErrTxNotFound (a tx outside the window), ErrCorruptedData,
// ahtree.ErrUnexistentData as a status error.
func (pt *ProofTree) DualProofBatch(src, tgt []*TxHeader, firstTx uint64,
	alh, inner [][sha256.Size]byte) (msgs [][]byte, errs []error, err error) {
	n := len(src)
	if len(tgt) != n || len(inner) != len(alh) {
		return nil, nil, ErrIllegalArguments
	}
	if n == 0 {
		return nil, nil, nil
	}
	for p := 0; p < n; p++ {
		if src[p] == nil || tgt[p] == nil { // immustore.go:2395-2397
			return nil, nil, ErrIllegalArguments
		}
	}
	blob := make([]byte, 0, 64)
	sh, th := packHeaders(src, &blob), packHeaders(tgt, &blob)
	blob = append(blob, 0)
	var ap, ip *C.uint8_t
	if len(alh) > 0 {
		ap, ip = (*C.uint8_t)(unsafe.Pointer(&alh[0][0])), (*C.uint8_t)(unsafe.Pointer(&inner[0][0]))
	}
	off := make([]uint64, n+1)
	status := make([]int32, n)
	out := make([]byte, 4096*n)
	for try := 0; try < 2; try++ {
		st := C.mh_ahtree_dual_proof_pb_batch(pt.t, C.uint64_t(n), &sh[0], &th[0],
			(*C.uint8_t)(unsafe.Pointer(&blob[0])), C.uint64_t(len(blob)-1), C.uint64_t(firstTx),
			C.uint64_t(len(alh)), ap, ip, (*C.uint8_t)(unsafe.Pointer(&out[0])), C.uint64_t(len(out)),
			(*C.uint64_t)(unsafe.Pointer(&off[0])), (*C.int32_t)(unsafe.Pointer(&status[0])))
		if st == C.MH_ERR_BUFFER_TOO_SMALL && try == 0 {
			out = make([]byte, off[n]+1) // the size query: off[n] is the total
			continue
		}
		if st != C.MH_OK {
			return nil, nil, mapErr(st)
		}
		break
	}
	msgs = make([][]byte, n)
	errs = make([]error, n)
	for p := 0; p < n; p++ {
		if status[p] != 0 {
			errs[p] = mapProofErr(C.int(status[p]))
			continue
		}
		msgs[p] = out[off[p]:off[p+1]]
	}
	return msgs, errs, nil
}

// packDualProofMessages lays the messages of a batch end to end, as the C
// calls read them (message p = buf[off[p]:off[p+1]]).
func packDualProofMessages(msgs [][]byte) (buf []byte, off []uint64) {
	off = make([]uint64, len(msgs)+1)
	total := 0
	for _, m := range msgs {
		total += len(m)
	}
	buf = make([]byte, 0, total+1)
	for p, m := range msgs {
		buf = append(buf, m...)
		off[p+1] = uint64(len(buf))
	}
	return append(buf, 0), off
}

// VerifyDualProofMessages is what pkg/client does with every VerifiableGet /
// VerifiableSet / VerifiableTxById answer (client.go:1090-1117, 1150-1213) --
// proto.Unmarshal, schema.DualProofFromProto, store.VerifyDualProof
// (verification.go:127-235) -- for a batch of marshalled schema.DualProof
// messages in one device pass: the messages go up once, one verdict each comes
// back.  ok[p] is VerifyDualProof(proof p, src[p], tgt[p], srcAlh[p],
// tgtAlh[p]); a message that does not decode (ErrCorruptedData at
// client.go:1112-1114) or lacks a header or its linear proof is false.  A
// message without LinearAdvanceProof is verified as it stands: nothing is
// fetched, FillMissingLinearAdvanceProof stays with the caller.
func VerifyDualProofMessages(msgs [][]byte, src, tgt []uint64,
	srcAlh, tgtAlh [][sha256.Size]byte) (ok []bool, err error) {
	return verifyDualProofMessages(msgs, src, tgt, srcAlh, tgtAlh, false)
}

// VerifyDualProofMessagesClique is VerifyDualProofMessages over every GPU of
// the process: the batch cut into parts of nearly equal message bytes, one
// per device over its own link (mh_multi_verify_dual_proof_pb_batch), on a
// clique checked out of the process's pool.
func VerifyDualProofMessagesClique(msgs [][]byte, src, tgt []uint64,
	srcAlh, tgtAlh [][sha256.Size]byte) (ok []bool, err error) {
	return verifyDualProofMessages(msgs, src, tgt, srcAlh, tgtAlh, true)
}

func verifyDualProofMessages(msgs [][]byte, src, tgt []uint64,
	srcAlh, tgtAlh [][sha256.Size]byte, clique bool) ([]bool, error) {
	n := len(msgs)
	if len(src) != n || len(tgt) != n || len(srcAlh) != n || len(tgtAlh) != n {
		return nil, ErrIllegalArguments
	}
	if n == 0 {
		return nil, nil
	}
	buf, off := packDualProofMessages(msgs)
	status := make([]int32, n)
	verdict := make([]uint8, n)
	var st C.int
	if clique {
		m, e := mi355x.AcquireClique()
		if e != nil {
			return nil, e
		}
		st = C.mh_multi_verify_dual_proof_pb_batch((*C.mh_multi)(m), C.uint64_t(n),
			(*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
			(*C.uint64_t)(unsafe.Pointer(&src[0])), (*C.uint64_t)(unsafe.Pointer(&tgt[0])),
			(*C.uint8_t)(unsafe.Pointer(&srcAlh[0][0])), (*C.uint8_t)(unsafe.Pointer(&tgtAlh[0][0])),
			(*C.int32_t)(unsafe.Pointer(&status[0])), (*C.uint8_t)(unsafe.Pointer(&verdict[0])))
		mi355x.ReleaseClique(m, int(st))
	} else {
		p, e := mi355x.Context()
		if e != nil {
			return nil, e
		}
		st = C.mh_verify_dual_proof_pb_batch((*C.mh_ctx)(p), C.uint64_t(n),
			(*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint64_t)(unsafe.Pointer(&off[0])),
			(*C.uint64_t)(unsafe.Pointer(&src[0])), (*C.uint64_t)(unsafe.Pointer(&tgt[0])),
			(*C.uint8_t)(unsafe.Pointer(&srcAlh[0][0])), (*C.uint8_t)(unsafe.Pointer(&tgtAlh[0][0])),
			(*C.int32_t)(unsafe.Pointer(&status[0])), (*C.uint8_t)(unsafe.Pointer(&verdict[0])))
	}
	if st != C.MH_OK {
		return nil, mapErr(st)
	}
	ok := make([]bool, n)
	for p := range ok {
		ok[p] = status[p] == 0 && verdict[p] != 0
	}
	return ok, nil
}

// VerifiedGetRequest and VerifiedGetState are the fields of
// schema.KeyRequest and schema.ImmutableState that verifiedGet reads
// (client.go:1130-1191), in plain types: pkg/api/schema imports this package,
// so it cannot be named here.  A caller in pkg/client fills them from kReq.Key
// / kReq.AtTx and state.TxId / state.TxHash.
type VerifiedGetRequest struct {
	Key  []byte // kReq.Key, without the set-key prefix
	AtTx uint64 // kReq.AtTx
}

type VerifiedGetState struct {
	TxID   uint64 // state.TxId; 0: no state yet
	TxHash []byte // state.TxHash; DigestFromProto: at most 32 bytes count
}

// VerifyVerifiableEntries is what pkg/client's verifiedGet does with every
// VerifiableGet answer before the state signature check (client.go:1140-1220)
// -- proto.Unmarshal into schema.VerifiableEntry, EncodeEntrySpec /
// EncodeReference, EntrySpecDigestFor, htree.VerifyInclusion, the choice of
// source and target, store.VerifyDualProof -- for a batch of marshalled answers
// in one device pass over the clique's GPUs
// (mh_multi_verify_verifiable_entry_pb_batch): answers, keys and states go up
// once, one status, one verdict and the new state come back per answer.
// errs[p] is nil and newStates[p] the state verifiedGet would store, or the
// error it would return: ErrCorruptedData where the proofs do not verify
// (client.go:1198) or the answer does not decode, ErrIllegalArguments where Go
// would dereference a nil part of the answer, ErrUnsupportedTxVersion from
// EntrySpecDigestFor.  A missing LinearAdvanceProof is verified as it stands:
// FillMissingLinearAdvanceProof stays with the caller.
func VerifyVerifiableEntries(answers [][]byte, reqs []VerifiedGetRequest,
	states []VerifiedGetState) (newStates []VerifiedGetState, errs []error, err error) {
	n := len(answers)
	if len(reqs) != n || len(states) != n {
		return nil, nil, ErrIllegalArguments
	}
	if n == 0 {
		return nil, nil, nil
	}
	buf, off := packDualProofMessages(answers)
	keyOff := make([]uint64, n+1)
	atTx := make([]uint64, n)
	stateTx := make([]uint64, n)
	stateAlh := make([][sha256.Size]byte, n)
	total := 0
	for _, r := range reqs {
		total += len(r.Key)
	}
	keys := make([]byte, 0, total+1)
	for p := range reqs {
		keys = append(keys, reqs[p].Key...)
		keyOff[p+1] = uint64(len(keys))
		atTx[p], stateTx[p] = reqs[p].AtTx, states[p].TxID
		copy(stateAlh[p][:], states[p].TxHash) // DigestFromProto (database_protoconv.go:293-297)
	}
	keys = append(keys, 0)
	status := make([]int32, n)
	verdict := make([]uint8, n)
	newTx := make([]uint64, n)
	newAlh := make([][sha256.Size]byte, n)
	// the batch struct lives in C memory: cgo forbids passing a Go pointer to
	// Go memory that itself holds Go pointers
	b := (*C.mh_verified_get_batch)(C.calloc(1, C.size_t(unsafe.Sizeof(C.mh_verified_get_batch{}))))
	if b == nil {
		return nil, nil, ErrIllegalState
	}
	defer C.free(unsafe.Pointer(b))
	var pin runtime.Pinner
	defer pin.Unpin()
	for _, ptr := range []unsafe.Pointer{unsafe.Pointer(&buf[0]), unsafe.Pointer(&off[0]),
		unsafe.Pointer(&keys[0]), unsafe.Pointer(&keyOff[0]), unsafe.Pointer(&atTx[0]),
		unsafe.Pointer(&stateTx[0]), unsafe.Pointer(&stateAlh[0][0])} {
		pin.Pin(ptr)
	}
	b.n = C.uint64_t(n)
	b.msgs, b.msg_off = (*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint64_t)(unsafe.Pointer(&off[0]))
	b.keys, b.key_off = (*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.uint64_t)(unsafe.Pointer(&keyOff[0]))
	b.at_tx, b.state_tx = (*C.uint64_t)(unsafe.Pointer(&atTx[0])), (*C.uint64_t)(unsafe.Pointer(&stateTx[0]))
	b.state_alh = (*C.uint8_t)(unsafe.Pointer(&stateAlh[0][0]))
	m, e := mi355x.AcquireClique()
	if e != nil {
		return nil, nil, e
	}
	st := C.mh_multi_verify_verifiable_entry_pb_batch((*C.mh_multi)(m), b,
		(*C.int32_t)(unsafe.Pointer(&status[0])), (*C.uint8_t)(unsafe.Pointer(&verdict[0])),
		(*C.uint64_t)(unsafe.Pointer(&newTx[0])), (*C.uint8_t)(unsafe.Pointer(&newAlh[0][0])))
	mi355x.ReleaseClique(m, int(st))
	if st != C.MH_OK {
		return nil, nil, mapErr(st)
	}
	newStates = make([]VerifiedGetState, n)
	errs = make([]error, n)
	for p := 0; p < n; p++ {
		switch {
		case status[p] == C.MH_ERR_UNSUPPORTED_TX_VERSION:
			errs[p] = ErrUnsupportedTxVersion // immustore.go:90, from EntrySpecDigestFor
		case status[p] != 0:
			errs[p] = mapErr(C.int(status[p]))
		case verdict[p] == 0:
			errs[p] = ErrCorruptedData // client.go:1198, and verifyDualProof's error
		default:
			newStates[p] = VerifiedGetState{TxID: newTx[p], TxHash: append([]byte(nil), newAlh[p][:]...)}
		}
	}
	return newStates, errs, nil
}

// VerifiedTxKind names the client call a VerifiableTx answer belongs to
// (MH_VTX_* of immustore_merkle.h, in that order).
type VerifiedTxKind uint8

const (
	VerifiedTxSet       VerifiedTxKind = iota // VerifiedSet, client.go:1302
	VerifiedTxSetAll                          // streamVerifiedSet, streams.go:128
	VerifiedTxReference                       // VerifiedSetReferenceAt, client.go:1677
	VerifiedTxZAdd                            // VerifiedZAddAt, client.go:1842
	VerifiedTxByID                            // VerifiedTxByID, client.go:1527
)

// VerifiedTxKV is one key / value pair the client sent (schema.KeyValue).
type VerifiedTxKV struct {
	Key, Value []byte
}

// VerifiedTxRequest is what the client sent for one VerifiableTx answer, in
// plain types (pkg/api/schema imports this package).  Set: one KV.  SetAll:
// the KVs of the request, in order.  Reference: Key and ReferencedKey, AtTx.
// ZAdd: Set, Score, Key, AtTx (ZAddRequest).  ByID: Tx, the requested id.
type VerifiedTxRequest struct {
	Kind          VerifiedTxKind
	KVs           []VerifiedTxKV
	Key           []byte
	ReferencedKey []byte
	Set           []byte
	Score         float64
	AtTx          uint64
	Tx            uint64
}

// wrapZAddReferenceAt is database.WrapZAddReferenceAt (pkg/database/meta.go:
// 98-117) over database.EncodeKey(key), as VerifiedZAddAt builds the entry's
// key (client.go:1893-1897): pkg/database cannot be imported from here.
func wrapZAddReferenceAt(set []byte, score float64, key []byte, atTx uint64) []byte {
	zKey := make([]byte, 0, 1+8+len(set)+8+8+1+len(key)+8)
	zKey = append(zKey, 1) // SortedSetKeyPrefix
	zKey = binary.BigEndian.AppendUint64(zKey, uint64(len(set)))
	zKey = append(zKey, set...)
	zKey = binary.BigEndian.AppendUint64(zKey, math.Float64bits(score))
	zKey = binary.BigEndian.AppendUint64(zKey, uint64(1+len(key)))
	zKey = append(zKey, 0) // SetKeyPrefix
	zKey = append(zKey, key...)
	return binary.BigEndian.AppendUint64(zKey, atTx)
}

// VerifyVerifiableTxs is what pkg/client does with every schema.VerifiableTx
// answer before the state signature check -- VerifiedSet (client.go:1337-1391),
// streamVerifiedSet (streams.go:205-260), VerifiedSetReferenceAt
// (client.go:1716-1770), VerifiedZAddAt (:1882-1940), VerifiedTxByID
// (:1554-1583): proto.Unmarshal, TxFromProto with the hash tree of the wire's
// entries, the inclusion of what the client sent, the rebuilt Eh against the
// DualProof's target header, the new state's Alh, store.VerifyDualProof -- for
// a batch of marshalled answers in one device pass over the clique's GPUs
// (mh_multi_verify_verifiable_tx_pb_batch).  errs[p] is nil and newStates[p]
// the state the call would store, or the error it would return:
// ErrCorruptedData where a check fails or the answer does not decode,
// ErrIllegalArguments where Go would dereference a nil part of the answer,
// ErrUnsupportedTxVersion from EntrySpecDigestFor.  A missing
// LinearAdvanceProof is verified as it stands.
func VerifyVerifiableTxs(answers [][]byte, reqs []VerifiedTxRequest,
	states []VerifiedGetState) (newStates []VerifiedGetState, errs []error, err error) {
	n := len(answers)
	if len(reqs) != n || len(states) != n {
		return nil, nil, ErrIllegalArguments
	}
	if n == 0 {
		return nil, nil, nil
	}
	buf, off := packDualProofMessages(answers)
	kind := make([]uint8, n)
	specOff := make([]uint64, n+1)
	atTx := make([]uint64, n)
	stateTx := make([]uint64, n)
	stateAlh := make([][sha256.Size]byte, n)
	keyOff, valOff := []uint64{0}, []uint64{0}
	var keys, vals []byte
	spec := func(k, v []byte) {
		keys, vals = append(keys, k...), append(vals, v...)
		keyOff, valOff = append(keyOff, uint64(len(keys))), append(valOff, uint64(len(vals)))
	}
	for p := range reqs {
		r := &reqs[p]
		kind[p] = uint8(r.Kind)
		switch r.Kind {
		case VerifiedTxSet, VerifiedTxSetAll:
			if len(r.KVs) == 0 || (r.Kind == VerifiedTxSet && len(r.KVs) != 1) {
				return nil, nil, ErrIllegalArguments
			}
			for _, kv := range r.KVs {
				spec(kv.Key, kv.Value)
			}
		case VerifiedTxReference:
			spec(r.Key, r.ReferencedKey)
			atTx[p] = r.AtTx
		case VerifiedTxZAdd:
			spec(wrapZAddReferenceAt(r.Set, r.Score, r.Key, r.AtTx), nil)
		case VerifiedTxByID:
			atTx[p] = r.Tx
		default:
			return nil, nil, ErrIllegalArguments
		}
		specOff[p+1] = uint64(len(keyOff) - 1)
		stateTx[p] = states[p].TxID
		copy(stateAlh[p][:], states[p].TxHash) // DigestFromProto (database_protoconv.go:293-297)
	}
	keys, vals = append(keys, 0), append(vals, 0)
	status := make([]int32, n)
	verdict := make([]uint8, n)
	newTx := make([]uint64, n)
	newAlh := make([][sha256.Size]byte, n)
	// the batch struct lives in C memory: cgo forbids passing a Go pointer to
	// Go memory that itself holds Go pointers
	b := (*C.mh_verified_tx_batch)(C.calloc(1, C.size_t(unsafe.Sizeof(C.mh_verified_tx_batch{}))))
	if b == nil {
		return nil, nil, ErrIllegalState
	}
	defer C.free(unsafe.Pointer(b))
	var pin runtime.Pinner
	defer pin.Unpin()
	for _, ptr := range []unsafe.Pointer{unsafe.Pointer(&buf[0]), unsafe.Pointer(&off[0]),
		unsafe.Pointer(&kind[0]), unsafe.Pointer(&specOff[0]), unsafe.Pointer(&keys[0]),
		unsafe.Pointer(&keyOff[0]), unsafe.Pointer(&vals[0]), unsafe.Pointer(&valOff[0]),
		unsafe.Pointer(&atTx[0]), unsafe.Pointer(&stateTx[0]), unsafe.Pointer(&stateAlh[0][0])} {
		pin.Pin(ptr)
	}
	b.n = C.uint64_t(n)
	b.msgs, b.msg_off = (*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint64_t)(unsafe.Pointer(&off[0]))
	b.kind, b.spec_off = (*C.uint8_t)(unsafe.Pointer(&kind[0])), (*C.uint64_t)(unsafe.Pointer(&specOff[0]))
	b.keys, b.key_off = (*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.uint64_t)(unsafe.Pointer(&keyOff[0]))
	b.vals, b.val_off = (*C.uint8_t)(unsafe.Pointer(&vals[0])), (*C.uint64_t)(unsafe.Pointer(&valOff[0]))
	b.at_tx, b.state_tx = (*C.uint64_t)(unsafe.Pointer(&atTx[0])), (*C.uint64_t)(unsafe.Pointer(&stateTx[0]))
	b.state_alh = (*C.uint8_t)(unsafe.Pointer(&stateAlh[0][0]))
	m, e := mi355x.AcquireClique()
	if e != nil {
		return nil, nil, e
	}
	st := C.mh_multi_verify_verifiable_tx_pb_batch((*C.mh_multi)(m), b,
		(*C.int32_t)(unsafe.Pointer(&status[0])), (*C.uint8_t)(unsafe.Pointer(&verdict[0])),
		(*C.uint64_t)(unsafe.Pointer(&newTx[0])), (*C.uint8_t)(unsafe.Pointer(&newAlh[0][0])), nil)
	mi355x.ReleaseClique(m, int(st))
	if st != C.MH_OK {
		return nil, nil, mapErr(st)
	}
	newStates = make([]VerifiedGetState, n)
	errs = make([]error, n)
	for p := 0; p < n; p++ {
		switch {
		case status[p] == C.MH_ERR_UNSUPPORTED_TX_VERSION:
			errs[p] = ErrUnsupportedTxVersion // immustore.go:90, from EntrySpecDigestFor
		case status[p] != 0:
			errs[p] = mapErr(C.int(status[p]))
		case verdict[p] == 0:
			errs[p] = ErrCorruptedData // client.go:1338, 1356, 1363, 1367 and verifyDualProof's error
		default:
			newStates[p] = VerifiedGetState{TxID: newTx[p], TxHash: append([]byte(nil), newAlh[p][:]...)}
		}
	}
	return newStates, errs, nil
}
