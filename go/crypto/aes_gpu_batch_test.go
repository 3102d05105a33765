// +build gpu

// aes_gpu_batch_test.go -- NewAESBatch (aes_gpu.go): a peer table's AES objects built in one call, their
// keys derived on the GPUs.  Each batch-built AES must be the AES NewAES builds from the same secret and
// salt: a packet sealed by one opens under the other, on whichever member owns the slot.
package crypto

import (
	"testing"
)

func TestNewAESBatchMatchesNewAES(t *testing.T) {
	gg, err := NewGPUGroup([]int{0, 0}, 64)
	if err != nil {
		t.Fatal(err)
	}
	defer gg.Close()
	const peers = 40
	secrets, salts := make([][]byte, peers), make([][]byte, peers)
	for i := range secrets {
		secrets[i], salts[i] = make([]byte, 32), make([]byte, SaltLength)
		for k := range secrets[i] {
			secrets[i][k], salts[i][k] = byte(7*i+k), byte(3*i+5*k+1)
		}
	}
	batch, err := gg.NewAESBatch(secrets, salts)
	if err != nil || len(batch) != peers {
		t.Fatalf("NewAESBatch: %d %v", len(batch), err)
	}
	members := map[int]bool{}
	ip := []byte{10, 99, 0, 1}
	for i, a := range batch {
		members[a.Member()] = true
		one, err := gg.NewAES(secrets[i], salts[i])
		if err != nil {
			t.Fatal(err)
		}
		data := make([]byte, 1350+28)
		fillSlice(data[:1350])
		want := append([]byte(nil), data[:1350]...)
		if n, err := a.Encrypt(data, 1350, ip); err != nil || n != 1350+28 {
			t.Fatalf("peer %d: Encrypt %d %v", i, n, err)
		}
		if n, err := one.Decrypt(data, ip); err != nil || n != 1350 || string(data[:1350]) != string(want) {
			t.Fatalf("peer %d: the NewAES key does not open the NewAESBatch packet: %d %v", i, n, err)
		}
		if i > 0 { // and never under a neighbour's key
			if _, err := a.Encrypt(data, 1350, ip); err != nil {
				t.Fatal(err)
			}
			if _, err := batch[i-1].Decrypt(data, ip); err != errOpen {
				t.Fatalf("peer %d's packet opened under peer %d's key", i, i-1)
			}
		}
		if i >= 20 {
			break // 64 slots: 40 batch-built + 21 single ones
		}
	}
	if len(members) != 2 {
		t.Fatalf("the table's keys should spread over both members, got %v", members)
	}
	if _, err := gg.NewAESBatch(secrets[:1], salts[:2]); err == nil {
		t.Fatal("secrets and salts of different number must be refused")
	}
	if _, err := gg.NewAESBatch([][]byte{make([]byte, 31)}, [][]byte{make([]byte, 32)}); err == nil {
		t.Fatal("a 31-byte secret must be refused")
	}
	if out, err := gg.NewAESBatch(nil, nil); err != nil || out != nil {
		t.Fatal("an empty table is no error")
	}
}
